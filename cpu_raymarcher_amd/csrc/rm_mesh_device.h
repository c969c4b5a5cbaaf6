// rm_mesh_device.h -- what the two surface-nets meshers share on the device (rm_mesh.hip over a dense volume, rm_mesh_sparse.hip
// over 9 x 9 x 9 tiles): the cell record, the ballot ranks, the scan of the workgroup totals, the vertex position and the stores
// of a vertex and of a quad.  The rule is the contract of include/rm_raymarch.h ("meshes"); both files keep to it through these.
#pragma once
#include <hip/hip_runtime.h>

#include "rm_kernels.h"

namespace {

constexpr unsigned kBlock = RM_MESH_BLOCK, kWaves = kBlock / 64, kScan = RM_MESH_SCAN_STEP;
constexpr uint32_t kNone = 0xFFFFFFFFu;  // map: the point's cell has no vertex

// The cell of point l: whether it exists, its eight corner values (corner dx + 2 dy + 4 dz) and which of them are inside.
struct Cell {
    unsigned i, j, k;
    bool exists, finite;
    unsigned inside;  // bit c: corner c < iso (NaN: outside)
    __device__ bool mixed() const { return inside != 0u && inside != 255u; }
    __device__ bool active() const { return exists && finite && mixed(); }
    __device__ bool hole() const { return exists && !finite && mixed(); }
    // the lattice edge from the point towards +A changes side
    __device__ bool crosses(int A) const { return exists && (((inside >> (1 << A)) ^ inside) & 1u); }
};

// the other two axes of A in cyclic order, and the linear stride of an axis
__device__ __forceinline__ constexpr int axis_b(int A) { return A == 2 ? 0 : A + 1; }
__device__ __forceinline__ constexpr int axis_c(int A) { return A == 0 ? 2 : A - 1; }
// the four cells around the edge from the point towards +A exist: the point's own cell does, and it has a lower neighbour on B and C
__device__ __forceinline__ bool ring_exists(const Cell &c, int A) {
    const unsigned p[3] = {c.i, c.j, c.k};
    return c.exists && p[axis_b(A)] >= 1u && p[axis_c(A)] >= 1u;
}

// Wave ballots of up to three flags -> this lane's exclusive rank among the set flags of its workgroup, in thread order and
// flag order within a thread, and (all lanes) the workgroup's total.  `sums`: kWaves words of LDS.
template <int FLAGS>
__device__ __forceinline__ unsigned block_rank(const bool (&flag)[FLAGS], unsigned *sums, unsigned *total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned before = 0, all = 0;
#pragma unroll
    for (int f = 0; f < FLAGS; ++f) {
        const unsigned long long b = __ballot(flag[f]);
        before += static_cast<unsigned>(__popcll(b & below));
        all += static_cast<unsigned>(__popcll(b));
    }
    if (lane == 0) sums[wave] = all;
    __syncthreads();
    unsigned sum = 0;
#pragma unroll
    for (unsigned w = 0; w < kWaves; ++w) {
        if (w < wave) before += sums[w];
        sum += sums[w];
    }
    *total = sum;
    return before;
}

// inclusive scan over the kScan threads of the workgroup; *total: the sum of all of them.  `sums`: kScan / 64 words of LDS.
__device__ __forceinline__ unsigned scan_step(unsigned x, unsigned *sums, unsigned *total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) sums[wave] = x;
    __syncthreads();
    unsigned sum = 0;
#pragma unroll
    for (unsigned w = 0; w < kScan / 64; ++w) {
        if (w < wave) x += sums[w];
        sum += sums[w];
    }
    *total = sum;
    return x;
}

__global__ __launch_bounds__(kScan) void mesh_scan_kernel(uint32_t *totals, unsigned n_blocks, RmMeshInfo *info) {
    __shared__ unsigned s_sums[3][kScan / 64];
    uint32_t *tv = totals, *tq = totals + n_blocks, *th = totals + 2ull * n_blocks;
    unsigned long long vertices = 0, quads = 0, holes = 0;
    unsigned at = threadIdx.x;
    unsigned nv = at < n_blocks ? tv[at] : 0u, nq = at < n_blocks ? tq[at] : 0u, nh = at < n_blocks ? th[at] : 0u;
    for (unsigned base = 0; base < n_blocks; base += kScan, at += kScan) {
        const unsigned v = nv, q = nq, h = nh, next = at + kScan;
        if (base + kScan < n_blocks) {  // the next step's totals are on their way while this one is scanned
            nv = next < n_blocks ? tv[next] : 0u;
            nq = next < n_blocks ? tq[next] : 0u;
            nh = next < n_blocks ? th[next] : 0u;
        }
        unsigned sv, sq, sh;
        const unsigned iv = scan_step(v, s_sums[0], &sv), iq = scan_step(q, s_sums[1], &sq);
        scan_step(h, s_sums[2], &sh);
        if (at < n_blocks) {  // fewer than 2^32 quads in all (3 per point, 2^30 points): the offsets fit
            tv[at] = static_cast<uint32_t>(vertices + (iv - v));
            tq[at] = static_cast<uint32_t>(quads + (iq - q));
        }
        vertices += sv;
        quads += sq;
        holes += sh;
        __syncthreads();  // the next step writes s_sums again
    }
    if (threadIdx.x == 0) {
        info->n_vertices = static_cast<long long>(vertices);
        info->n_quads = static_cast<long long>(quads);
        info->n_holes = static_cast<long long>(holes);
        info->reserved = 0;
    }
}

// The vertex of an active cell: the mean of its edge crossings in the order of the rule (axis 0, 1, 2; within an axis the low
// end's offsets on the other two axes (0,0), (1,0), (0,1), (1,1), the lower-numbered axis first), then the lattice's point rule
// (rm_kernels.h, rm_lattice_component) with the fractional index.  binary64, one operation at a time (-ffp-contract=off), one
// rounding to binary32.
template <typename ARGS>
__device__ __forceinline__ void vertex_position(const ARGS &a, const Cell &c, const double (&v)[8], float out[3]) {
    double sum[3] = {0.0, 0.0, 0.0};
    unsigned m = 0;
#pragma unroll
    for (int A = 0; A < 3; ++A) {
        const int lo_axis = A == 0 ? 1 : 0, hi_axis = A == 2 ? 1 : 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int low = ((e & 1) << lo_axis) | ((e >> 1) << hi_axis), high = low | (1 << A);
            if (((c.inside >> low) ^ (c.inside >> high)) & 1u) {
                double at[3];
                at[A] = (a.iso - v[low]) / (v[high] - v[low]);
                at[lo_axis] = static_cast<double>(e & 1);
                at[hi_axis] = static_cast<double>(e >> 1);
                sum[0] = sum[0] + at[0];
                sum[1] = sum[1] + at[1];
                sum[2] = sum[2] + at[2];
                ++m;
            }
        }
    }
    const double count = static_cast<double>(m);
    const double fi = static_cast<double>(c.i) + sum[0] / count, fj = static_cast<double>(c.j) + sum[1] / count,
                 fk = static_cast<double>(c.k) + sum[2] / count;
#pragma unroll
    for (int n = 0; n < 3; ++n) out[n] = static_cast<float>(rm_lattice_component(a.lat, n, fi, fj, fk));
}

// the key of a cell: the linear index of its low corner in the lattice
template <typename ARGS>
__device__ __forceinline__ long long cell_key(const ARGS &a, const Cell &c) {
    return (static_cast<long long>(c.k) * a.nv + c.j) * a.nu + c.i;
}

// Vertex n of the mesh, the one of the active cell c, where the capacity has room for it; `cells` (may be null): its key too.
template <typename ARGS>
__device__ __forceinline__ void store_vertex(const ARGS &a, const Cell &c, const double (&v)[8], unsigned n, long long *cells) {
    if (static_cast<long long>(n) >= a.cap_vertices) return;
    float p[3];
    vertex_position(a, c, v, p);
    float *out = a.vertices + 3ull * n;
    out[0] = p[0];
    out[1] = p[1];
    out[2] = p[2];
    if (cells) cells[n] = cell_key(a, c);
}

// Quad q of the mesh where the capacity has room for it: the ring of the four cells' vertices around the edge from the point
// of cell c towards +A, counter-clockwise seen from +A when the point is inside; `edges` (may be null): its key 3 l + A too.
// (The loop over A stays with the kernels: in here it turns the ring into a run-time indexed vector, 40 VGPRs for 26.)
template <typename ARGS>
__device__ __forceinline__ void store_quad(const ARGS &a, const Cell &c, const uint32_t (&ring)[4], unsigned q, long long *edges, long long l, int A) {
    if (static_cast<long long>(q) >= a.cap_quads) return;
    const bool in = c.inside & 1u;
    uint32_t *out = a.quads + 4ull * q;
    out[0] = ring[0];
    out[1] = ring[in ? 1 : 3];
    out[2] = ring[2];
    out[3] = ring[in ? 3 : 1];
    if (edges) edges[q] = 3ll * l + A;
}

}  // namespace
