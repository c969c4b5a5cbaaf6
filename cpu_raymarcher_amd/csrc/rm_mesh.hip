// rm_mesh.hip -- naive surface nets on a lattice of distances (gfx950): rm_mesh_field_device and rm_scene_mesh.
//
// The rule is the contract of include/rm_raymarch.h ("meshes"); tests/mesh_model.py restates it in numpy and the results are
// compared byte for byte.  Work is mapped by lattice point: point l owns the cell whose low corner it is and the three lattice
// edges that leave it towards +i, +j, +k, so a workgroup of 256 threads covers 256 consecutive linear indices (a wave 64
// consecutive i of a row, the coalescing of field_kernel) and both orderings -- vertices by l, quads by 3 l + A -- are the
// order of the threads.  Four kernels on one stream, no host round trip:
//   mesh_count_kernel   per point: active cell, hole, quads (0 .. 3); wave ballots, one LDS word per wave, one total per block
//   mesh_scan_kernel    one workgroup: exclusive scan of the block totals in steps of RM_MESH_SCAN_STEP blocks (in place), the
//                       three totals into rm_mesh_info -- the same offsets on every run, nothing depends on arrival order
//   mesh_vertex_kernel  flags again, rank from ballots: the cell -> vertex map (one word per point) and the positions
//   mesh_quad_kernel    the crossing edges again; the four cells' vertices come from the map
// The overlapping corner loads of neighbouring lanes are left to the caches (DESIGN.md 4 says what was and was not measured).
#include <hip/hip_runtime.h>

#include "rm_mesh_device.h"

namespace {

template <typename T>
__device__ __forceinline__ double value_at(const RmMeshArgs &a, size_t l) {
    return static_cast<double>(static_cast<const T *>(a.values)[l]);  // binary32 widens exactly
}

__device__ __forceinline__ Cell locate(const RmMeshArgs &a, unsigned l) {
    Cell c;
    const unsigned row = l / a.nu;
    c.i = l - row * a.nu;
    c.k = row / a.nv;
    c.j = row - c.k * a.nv;
    c.exists = l < a.n && c.i + 1 < a.nu && c.j + 1 < a.nv && c.k + 1 < a.nw;
    c.finite = true;
    c.inside = 0;
    return c;
}

// CORNERS: 0xFF all eight, 0x17 the point and its three +neighbours (corners 0, 1, 2, 4: all the crossing test reads)
template <typename T, unsigned CORNERS>
__device__ __forceinline__ Cell load_cell(const RmMeshArgs &a, unsigned l, double v[8]) {
    Cell c = locate(a, l);
    if (c.exists) {
        const size_t sj = a.nu, sk = static_cast<size_t>(a.nu) * a.nv;
#pragma unroll
        for (unsigned n = 0; n < 8; ++n) {
            if (!((CORNERS >> n) & 1u)) continue;
            v[n] = value_at<T>(a, l + (n & 1u) + ((n >> 1) & 1u) * sj + (n >> 2) * sk);
            c.finite = c.finite && isfinite(v[n]);
            c.inside |= (v[n] < a.iso ? 1u : 0u) << n;
        }
    }
    return c;
}

__device__ __forceinline__ long long stride(const RmMeshArgs &a, int axis) {
    return axis == 0 ? 1ll : axis == 1 ? static_cast<long long>(a.nu) : static_cast<long long>(a.nu) * a.nv;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mesh_count_kernel(RmMeshArgs a) {
    __shared__ unsigned s_sums[3][kWaves];
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    double v[8];
    const Cell c = load_cell<T, 0xFFu>(a, l, v);
    bool quad[3];
#pragma unroll
    for (int A = 0; A < 3; ++A) {
        quad[A] = c.crosses(A) && ring_exists(c, A);
        if (quad[A]) {
            // Each of the four cells holds the crossing edge, so none is all inside or all outside: they are all active iff
            // their 18 corners -- 2 along A, 3 x 3 across -- are finite.
            const long long sa = stride(a, A), sb = stride(a, axis_b(A)), sc = stride(a, axis_c(A));
            bool finite = true;
            for (int n = 0; n < 18; ++n) {
                const long long at = static_cast<long long>(l) + (n & 1) * sa + ((n >> 1) % 3 - 1) * sb + ((n >> 1) / 3 - 1) * sc;
                finite = finite && isfinite(value_at<T>(a, static_cast<size_t>(at)));
            }
            quad[A] = finite;
        }
    }
    unsigned n_active, n_quads, n_holes;
    const bool act[1] = {c.active()}, hol[1] = {c.hole()};
    block_rank<1>(act, s_sums[0], &n_active);
    block_rank<3>(quad, s_sums[1], &n_quads);
    block_rank<1>(hol, s_sums[2], &n_holes);
    if (threadIdx.x == 0) {
        a.totals[blockIdx.x] = n_active;
        a.totals[a.n_blocks + blockIdx.x] = n_quads;
        a.totals[2ull * a.n_blocks + blockIdx.x] = n_holes;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mesh_vertex_kernel(RmMeshArgs a) {
    __shared__ unsigned s_sums[kWaves];
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    double v[8];
    const Cell c = load_cell<T, 0xFFu>(a, l, v);
    const bool act[1] = {c.active()};
    unsigned total;
    const unsigned r = a.totals[blockIdx.x] + block_rank<1>(act, s_sums, &total);
    if (l < a.n) a.map[l] = act[0] ? r : kNone;
    if (act[0]) store_vertex(a, c, v, r, nullptr);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mesh_quad_kernel(RmMeshArgs a) {
    __shared__ unsigned s_sums[kWaves];
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    double v[8];
    const Cell c = load_cell<T, 0x17u>(a, l, v);
    bool quad[3];
    uint32_t ring[3][4];
#pragma unroll
    for (int A = 0; A < 3; ++A) {
        quad[A] = c.crosses(A) && ring_exists(c, A);
        if (quad[A]) {  // c0 = p - e_B - e_C, c1 = p - e_C, c2 = p, c3 = p - e_B: all four active
            const long long sb = stride(a, axis_b(A)), sc = stride(a, axis_c(A));
            ring[A][0] = a.map[l - sb - sc];
            ring[A][1] = a.map[l - sc];
            ring[A][2] = a.map[l];
            ring[A][3] = a.map[l - sb];
            quad[A] = ring[A][0] != kNone && ring[A][1] != kNone && ring[A][2] != kNone && ring[A][3] != kNone;
        }
    }
    unsigned total;
    unsigned q = a.totals[a.n_blocks + blockIdx.x] + block_rank<3>(quad, s_sums, &total);
#pragma unroll
    for (int A = 0; A < 3; ++A) {
        if (!quad[A]) continue;
        store_quad(a, c, ring[A], q, nullptr, 0, A);
        ++q;
    }
}

// rm_mesh_cells_device: mesh_vertex_kernel's flags and ranks, the cell's key l where that kernel writes the position
template <typename T>
__global__ __launch_bounds__(kBlock) void cell_keys_kernel(RmMeshArgs a, long long *cells) {
    __shared__ unsigned s_sums[kWaves];
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    double v[8];
    const Cell c = load_cell<T, 0xFFu>(a, l, v);
    const bool act[1] = {c.active()};
    unsigned total;
    const unsigned r = a.totals[blockIdx.x] + block_rank<1>(act, s_sums, &total);
    if (act[0] && static_cast<long long>(r) < a.cap_vertices) cells[r] = static_cast<long long>(l);
}

template <typename T>
hipError_t launch_cells(const RmMeshArgs &a, long long *cells, hipStream_t stream) {
    const dim3 grid(a.n_blocks), block(kBlock);
    hipLaunchKernelGGL(mesh_count_kernel<T>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kScan), 0, stream, a.totals, a.n_blocks, a.info);
    if (a.cap_vertices > 0) hipLaunchKernelGGL(cell_keys_kernel<T>, grid, block, 0, stream, a, cells);
    return hipGetLastError();
}

template <typename T>
hipError_t launch(const RmMeshArgs &a, hipStream_t stream) {
    const dim3 grid(a.n_blocks), block(kBlock);
    hipLaunchKernelGGL(mesh_count_kernel<T>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kScan), 0, stream, a.totals, a.n_blocks, a.info);
    if (a.cap_vertices > 0 || a.cap_quads > 0) hipLaunchKernelGGL(mesh_vertex_kernel<T>, grid, block, 0, stream, a);
    if (a.cap_quads > 0) hipLaunchKernelGGL(mesh_quad_kernel<T>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rm_launch_mesh(const RmMeshArgs &a, hipStream_t stream, const char **kernel_name) {
    if (a.n <= 0 || a.n > (1ll << 30) || a.n_blocks != static_cast<unsigned>((a.n + kBlock - 1) / kBlock)) return hipErrorInvalidValue;
    if (kernel_name) *kernel_name = a.f32 ? "mesh_count_kernel<float>" : "mesh_count_kernel<double>";
    return a.f32 ? launch<float>(a, stream) : launch<double>(a, stream);
}

hipError_t rm_launch_mesh_cells(const RmMeshArgs &a, long long *cells, hipStream_t stream, const char **kernel_name) {
    if (a.n <= 0 || a.n > (1ll << 30) || a.n_blocks != static_cast<unsigned>((a.n + kBlock - 1) / kBlock)) return hipErrorInvalidValue;
    if (a.cap_vertices > 0 && !cells) return hipErrorInvalidValue;
    if (kernel_name) *kernel_name = a.f32 ? "mesh_count_kernel<float>" : "mesh_count_kernel<double>";
    return a.f32 ? launch_cells<float>(a, cells, stream) : launch_cells<double>(a, cells, stream);
}
