// rm_mesh_sparse.hip -- surface nets over the 9 x 9 x 9 tiles of the kept blocks of a lattice (gfx950): the compaction of
// rm_scene_blocks_device and rm_mesh_tiles_device.
//
// The rule is the contract of include/rm_raymarch.h ("sparse meshes"); tests/mesh_sparse_model.py restates it in numpy and the
// results are compared byte for byte.  Inside / active / hole, the vertex position, the quad ring and the winding are the dense
// mesher's, through the functions of rm_mesh_device.h.  Work is mapped by kept block: workgroup r of 256 threads takes the block
// of slot r, stages its tile once in LDS (729 binary64 values, 5 832 bytes) and gives lane t the cells of local index t and
// t + 256, so the order of the rule -- vertices by (slot, local cell), quads by (slot, 3 local + A) -- is the order of the
// workgroups, the two halves and the threads.  Cells of neighbouring blocks are reached through the slot map: their corner
// values in the neighbour's tile (count), their vertices in the neighbour's part of the cell -> vertex map (quads).
//   blocks_scan_kernel / blocks_scatter_kernel   the coarse pass's keep flags -> ranks and the list, in block order
//   mesh_tiles_count_kernel    per kept block: active cells, quads and holes
//   mesh_scan_kernel           the dense mesher's scan (rm_mesh_device.h) over one total per kept block
//   mesh_tiles_vertex_kernel   the map (one word per cell of a kept block), the positions, the cells' fine linear indices
//   mesh_tiles_quad_kernel     the crossing edges again; the four cells' vertices come from the map
#include "rm_mesh_device.h"

namespace {

constexpr unsigned kTile = RM_SPARSE_TILE, kCells = RM_SPARSE_CELLS, kB = RM_SPARSE_BLOCK;

// ---- the coarse pass: totals of kept blocks per workgroup of 256 blocks -> offsets, n_kept; flags -> ranks and the list

__global__ __launch_bounds__(kScan) void blocks_scan_kernel(uint32_t *totals, unsigned n_groups, RmSparseInfo *info, unsigned n_blocks) {
    __shared__ unsigned s_sums[kScan / 64];
    unsigned long long kept = 0;
    for (unsigned base = 0; base < n_groups; base += kScan) {
        const unsigned at = base + threadIdx.x;
        const unsigned v = at < n_groups ? totals[at] : 0u;
        unsigned sum;
        const unsigned inc = scan_step(v, s_sums, &sum);
        if (at < n_groups) totals[at] = static_cast<uint32_t>(kept + (inc - v));  // at most 2^24 blocks: the offsets fit
        kept += sum;
        __syncthreads();  // the next step writes s_sums again
    }
    if (threadIdx.x == 0) {
        info->n_blocks = static_cast<long long>(n_blocks);
        info->n_kept = static_cast<long long>(kept);
        info->reserved[0] = 0;
        info->reserved[1] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void blocks_scatter_kernel(RmBlocksArgs a) {
    __shared__ unsigned s_sums[kWaves];
    const unsigned b = blockIdx.x * kBlock + threadIdx.x;
    const bool keep[1] = {b < a.n_blocks && a.slot[b] == 0};
    unsigned total;
    const unsigned r = a.totals[blockIdx.x] + block_rank<1>(keep, s_sums, &total);
    if (keep[0]) {
        a.slot[b] = static_cast<int32_t>(r);
        a.list[r] = static_cast<int32_t>(b);
    }
}

// ---- the mesher

// The block of slot r: its coordinates and how many of its 8 cells per axis exist (0 for a list entry outside the lattice).
struct Block {
    unsigned bx, by, bz, cx, cy, cz;
};
__device__ __forceinline__ unsigned cells_on_axis(unsigned n, unsigned b) {
    const unsigned first = kB * b;
    return (n >= 2u && first < n - 1u) ? min(kB, n - 1u - first) : 0u;
}
__device__ __forceinline__ Block block_of_slot(const RmSparseMeshArgs &a, unsigned r) {
    const unsigned b = static_cast<unsigned>(a.list[r]);
    Block k;
    const unsigned row = b / a.nbu;
    k.bx = b - row * a.nbu;
    k.bz = row / a.nbv;
    k.by = row - k.bz * a.nbv;
    const bool in = k.bz < a.nbw;
    k.cx = in ? cells_on_axis(a.nu, k.bx) : 0u;
    k.cy = in ? cells_on_axis(a.nv, k.by) : 0u;
    k.cz = in ? cells_on_axis(a.nw, k.bz) : 0u;
    return k;
}

__device__ __forceinline__ void stage_tile(const RmSparseMeshArgs &a, unsigned r, double *s_tile) {
    const double *src = a.tiles + static_cast<size_t>(r) * kTile;
    for (unsigned t = threadIdx.x; t < kTile; t += kBlock) s_tile[t] = src[t];
    __syncthreads();
}

__device__ __forceinline__ unsigned tile_at(unsigned x, unsigned y, unsigned z) { return (z * 9u + y) * 9u + x; }

// The cell of local index `local` of the staged block, as the dense mesher's load_cell gives it.
template <unsigned CORNERS>
__device__ __forceinline__ Cell load_local(const RmSparseMeshArgs &a, const Block &k, const double *s_tile, unsigned local, double v[8]) {
    const unsigned x = local & 7u, y = (local >> 3) & 7u, z = local >> 6;
    Cell c;
    c.i = kB * k.bx + x;
    c.j = kB * k.by + y;
    c.k = kB * k.bz + z;
    c.exists = x < k.cx && y < k.cy && z < k.cz;
    c.finite = true;
    c.inside = 0;
    if (c.exists) {
#pragma unroll
        for (unsigned n = 0; n < 8; ++n) {
            if (!((CORNERS >> n) & 1u)) continue;
            v[n] = s_tile[tile_at(x + (n & 1u), y + ((n >> 1) & 1u), z + (n >> 2))];
            c.finite = c.finite && isfinite(v[n]);
            c.inside |= (v[n] < a.iso ? 1u : 0u) << n;
        }
    }
    return c;
}

// the slot of the block that holds cell (i, j, k) -- an existing cell --, or -1 when that block was not kept
__device__ __forceinline__ int slot_of_cell(const RmSparseMeshArgs &a, unsigned i, unsigned j, unsigned k) {
    const int s = a.slot[(static_cast<size_t>(k >> 3) * a.nbv + (j >> 3)) * a.nbu + (i >> 3)];
    return (s >= 0 && static_cast<unsigned>(s) < a.n_kept) ? s : -1;
}

// Cell (i, j, k) exists and holds an edge that changes side: it is active iff its block was kept and its eight corners, read
// from that block's tile (the staged one when it is this workgroup's), are finite.
__device__ __forceinline__ bool crossed_cell_active(const RmSparseMeshArgs &a, const Block &own, const double *s_tile, unsigned i, unsigned j,
                                                    unsigned k) {
    const unsigned x = i & 7u, y = j & 7u, z = k & 7u;
    const bool mine = (i >> 3) == own.bx && (j >> 3) == own.by && (k >> 3) == own.bz;
    const double *tile = s_tile;
    if (!mine) {
        const int s = slot_of_cell(a, i, j, k);
        if (s < 0) return false;
        tile = a.tiles + static_cast<size_t>(s) * kTile;
    }
    bool finite = true;
#pragma unroll
    for (unsigned n = 0; n < 8; ++n) finite = finite && isfinite(tile[tile_at(x + (n & 1u), y + ((n >> 1) & 1u), z + (n >> 2))]);
    return finite;
}

// cell c - e_B * db - e_C * dc for the ring of axis A
__device__ __forceinline__ void ring_cell(const Cell &c, int A, unsigned db, unsigned dc, unsigned out[3]) {
    out[0] = c.i;
    out[1] = c.j;
    out[2] = c.k;
    out[axis_b(A)] -= db;
    out[axis_c(A)] -= dc;
}

__global__ __launch_bounds__(kBlock) void mesh_tiles_count_kernel(RmSparseMeshArgs a) {
    __shared__ double s_tile[kTile];
    __shared__ unsigned s_sums[3][kWaves];
    const unsigned r = blockIdx.x;
    const Block k = block_of_slot(a, r);
    stage_tile(a, r, s_tile);
    bool act[2], hol[2], quad[6];
#pragma unroll
    for (unsigned h = 0; h < 2; ++h) {
        double v[8];
        const Cell c = load_local<0xFFu>(a, k, s_tile, threadIdx.x + h * kBlock, v);
        act[h] = c.active();
        hol[h] = c.hole();
#pragma unroll
        for (int A = 0; A < 3; ++A) {
            bool q = c.crosses(A) && ring_exists(c, A) && c.finite;
            if (q) {  // c0 = p - e_B - e_C, c1 = p - e_C, c3 = p - e_B: each holds the crossing edge
                unsigned n[3];
                ring_cell(c, A, 1, 1, n);
                q = crossed_cell_active(a, k, s_tile, n[0], n[1], n[2]);
                ring_cell(c, A, 0, 1, n);
                q = q && crossed_cell_active(a, k, s_tile, n[0], n[1], n[2]);
                ring_cell(c, A, 1, 0, n);
                q = q && crossed_cell_active(a, k, s_tile, n[0], n[1], n[2]);
            }
            quad[3 * h + A] = q;
        }
    }
    unsigned n_active, n_quads, n_holes;
    block_rank<2>(act, s_sums[0], &n_active);
    block_rank<6>(quad, s_sums[1], &n_quads);
    block_rank<2>(hol, s_sums[2], &n_holes);
    if (threadIdx.x == 0) {
        a.totals[r] = n_active;
        a.totals[a.n_kept + r] = n_quads;
        a.totals[2ull * a.n_kept + r] = n_holes;
    }
}

__global__ __launch_bounds__(kBlock) void mesh_tiles_vertex_kernel(RmSparseMeshArgs a) {
    __shared__ double s_tile[kTile];
    __shared__ unsigned s_sums[2][kWaves];
    const unsigned r = blockIdx.x;
    const Block k = block_of_slot(a, r);
    stage_tile(a, r, s_tile);
    unsigned first = a.totals[r];  // the vertices of this block; its second half follows its first
#pragma unroll
    for (unsigned h = 0; h < 2; ++h) {
        const unsigned local = threadIdx.x + h * kBlock;
        double v[8];
        const Cell c = load_local<0xFFu>(a, k, s_tile, local, v);
        const bool act[1] = {c.active()};
        unsigned total;
        const unsigned n = first + block_rank<1>(act, s_sums[h], &total);
        first += total;
        a.map[static_cast<size_t>(r) * kCells + local] = act[0] ? n : kNone;
        if (act[0]) store_vertex(a, c, v, n, a.cells);
    }
}

// the vertex of cell (i, j, k) -- an existing cell --, or kNone: its block was not kept, or the cell is not active
__device__ __forceinline__ uint32_t vertex_of(const RmSparseMeshArgs &a, const unsigned n[3]) {
    const int s = slot_of_cell(a, n[0], n[1], n[2]);
    if (s < 0) return kNone;
    return a.map[static_cast<size_t>(s) * kCells + ((n[2] & 7u) * kB + (n[1] & 7u)) * kB + (n[0] & 7u)];
}

__global__ __launch_bounds__(kBlock) void mesh_tiles_quad_kernel(RmSparseMeshArgs a) {
    __shared__ double s_tile[kTile];
    __shared__ unsigned s_sums[2][kWaves];
    const unsigned r = blockIdx.x;
    const Block k = block_of_slot(a, r);
    stage_tile(a, r, s_tile);
    unsigned first = a.totals[a.n_kept + r];
#pragma unroll
    for (unsigned h = 0; h < 2; ++h) {
        const unsigned local = threadIdx.x + h * kBlock;
        double v[8];
        const Cell c = load_local<0x17u>(a, k, s_tile, local, v);
        bool quad[3];
        uint32_t ring[3][4];
#pragma unroll
        for (int A = 0; A < 3; ++A) {
            quad[A] = c.crosses(A) && ring_exists(c, A);
            if (quad[A]) {  // c0 = p - e_B - e_C, c1 = p - e_C, c2 = p, c3 = p - e_B: all four active
                unsigned n[3];
                ring_cell(c, A, 1, 1, n);
                ring[A][0] = vertex_of(a, n);
                ring_cell(c, A, 0, 1, n);
                ring[A][1] = vertex_of(a, n);
                ring[A][2] = a.map[static_cast<size_t>(r) * kCells + local];
                ring_cell(c, A, 1, 0, n);
                ring[A][3] = vertex_of(a, n);
                quad[A] = ring[A][0] != kNone && ring[A][1] != kNone && ring[A][2] != kNone && ring[A][3] != kNone;
            }
        }
        unsigned total;
        unsigned q = first + block_rank<3>(quad, s_sums[h], &total);
        first += total;
        const long long l = cell_key(a, c);
#pragma unroll
        for (int A = 0; A < 3; ++A) {
            if (!quad[A]) continue;
            store_quad(a, c, ring[A], q, a.edges, l, A);
            ++q;
        }
    }
}

// rm_scene_tiles_update_device: the flags of the kept blocks (1: the previous tile was copied) -> info.  One workgroup, plain
// sums of integers: nothing depends on arrival order.
__global__ __launch_bounds__(kScan) void tiles_update_totals_kernel(const int32_t *reused, unsigned n_kept, RmTilesUpdateInfo *info) {
    __shared__ unsigned s_sums[kScan / 64];
    unsigned mine = 0;
    for (unsigned at = threadIdx.x; at < n_kept; at += kScan) mine += reused[at] != 0 ? 1u : 0u;
    unsigned total;
    scan_step(mine, s_sums, &total);
    if (threadIdx.x == 0) {
        info->n_kept = static_cast<long long>(n_kept);
        info->n_reused = static_cast<long long>(total);
        info->n_evaluated = static_cast<long long>(n_kept - total);
        info->reserved = 0;
    }
}

}  // namespace

hipError_t rm_launch_tiles_update_totals(const int32_t *reused, unsigned int n_kept, RmTilesUpdateInfo *info, hipStream_t stream) {
    hipLaunchKernelGGL(tiles_update_totals_kernel, dim3(1), dim3(kScan), 0, stream, reused, n_kept, info);
    return hipGetLastError();
}

hipError_t rm_launch_blocks_compact(const RmBlocksArgs &a, hipStream_t stream) {
    if (a.n_blocks == 0 || a.n_blocks > RM_SPARSE_MAX_BLOCKS || a.n_groups != (a.n_blocks + kBlock - 1) / kBlock) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blocks_scan_kernel, dim3(1), dim3(kScan), 0, stream, a.totals, a.n_groups, a.info, a.n_blocks);
    hipLaunchKernelGGL(blocks_scatter_kernel, dim3(a.n_groups), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t rm_launch_mesh_tiles(const RmSparseMeshArgs &a, hipStream_t stream, const char **kernel_name) {
    if (a.n_kept == 0 || a.n_kept > RM_SPARSE_MAX_KEPT) return hipErrorInvalidValue;
    if (kernel_name) *kernel_name = "mesh_tiles_count_kernel";
    const dim3 grid(a.n_kept), block(kBlock);
    hipLaunchKernelGGL(mesh_tiles_count_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kScan), 0, stream, a.totals, a.n_kept, a.info);
    if (a.cap_vertices > 0 || a.cap_quads > 0) hipLaunchKernelGGL(mesh_tiles_vertex_kernel, grid, block, 0, stream, a);
    if (a.cap_quads > 0) hipLaunchKernelGGL(mesh_tiles_quad_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}
