// rm_scene_build.hip -- the four pair loops of a sphere scene's build on the device (rm_scene_host.h, PairLoops): the
// nearest-candidate grid of a BVH scene, its exterior candidate grid, the sub-cell lists of crowded octree leaves, and the
// distance from every empty octree node to the nearest primitive box (octree.ts:155-160).  The host builder
// (rm_scene_host.cpp) is the definition: every kernel here evaluates the host's expressions, operation for operation, in
// binary64 -- this file is compiled with -ffp-contract=off like the host code, and binary64 division and square root are
// correctly rounded on both sides -- so the tables are the host's, byte for byte.  What is free is the ORDER: a minimum does
// not depend on it, and a list in increasing sphere order is the same list however the spheres were dealt to lanes.
//
// One wave per cell (or node), lanes striding the spheres (or boxes); four waves per workgroup.  Every index is checked
// against the count that came with its table.
#include <hip/hip_runtime.h>

#include "rm_kernels.h"

namespace {

constexpr int kWave = 64, kBlock = 256, kWavesPerBlock = kBlock / kWave;

// min over the wave in every lane; `o < v ? o : v` is the host's `if (d < best) best = d` (no NaN passes it)
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const double o = __shfl_xor(v, m, kWave);
        v = o < v ? o : v;
    }
    return v;
}

// rmh::js_hypot3, step by step: largest magnitude, the three quotients, the compensated sum, sqrt(sum) * big.  The
// arguments are any binary64 values (box_gap passes differences of binary32 numbers, which are not binary32 numbers), so
// none of the shortcuts of rm_device.h's hypot3(float, float, float) apply.
__device__ __forceinline__ double hypot3_f64(double x, double y, double z) {
    const double v[3] = {__builtin_fabs(x), __builtin_fabs(y), __builtin_fabs(z)};
    double big = 0.0;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (v[k] != v[k]) nan = true;
        else if (v[k] > big) big = v[k];
    }
    if (big == __builtin_inf()) return big;
    if (nan) return __builtin_nan("");
    if (big == 0.0) return 0.0;
    double sum = 0.0, comp = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double q = v[k] / big;
        const double term = q * q - comp;
        const double next = sum + term;
        comp = (next - sum) - term;
        sum = next;
    }
    return __builtin_sqrt(sum) * big;
}

struct CellBox {
    double lo[3], hi[3];
    int32_t first, n;  // the cell's spheres: entries [first, first + n) of ids, or of the sphere table without ids
};

// The box of cell `cell` (linear over all grids), grown by 3 % of a cell as the host grows it; false: no such cell.
__device__ __forceinline__ bool cell_box(const RmCandArgs &a, long long cell, CellBox &c) {
    if (a.cells_per_grid <= 0) return false;
    const long long g = cell / a.cells_per_grid;
    if (cell < 0 || g >= a.n_grids) return false;
    const RmCandGrid &G = a.grids[g];
    const int32_t local = static_cast<int32_t>(cell - g * a.cells_per_grid);
    if (G.dim[0] <= 0 || G.dim[1] <= 0 || G.dim[2] <= 0) return false;
    const int32_t ci[3] = {local % G.dim[0], (local / G.dim[0]) % G.dim[1], local / (G.dim[0] * G.dim[1])};
    if (ci[2] >= G.dim[2]) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.lo[k] = G.org[k] + (static_cast<double>(ci[k]) - 0.03) * G.w[k];
        c.hi[k] = G.org[k] + (static_cast<double>(ci[k]) + 1.03) * G.w[k];
    }
    c.first = G.first;
    c.n = G.n;
    return true;
}

// lb and ub of sphere j of the cell (rm_scene_host.cpp, build_point_query_grid has the rule); false: no such sphere
__device__ __forceinline__ bool cell_bounds(const RmCandArgs &a, const CellBox &c, int32_t j, double &lb, double &ub) {
    if (j < 0 || j >= c.n) return false;
    long long id = static_cast<long long>(c.first) + j;
    if (id < 0) return false;
    if (a.ids) {
        if (id >= a.n_ids) return false;
        id = a.ids[id];
    }
    if (id < 0 || id >= a.n_spheres) return false;
    const double *sp = a.spheres + 4 * id;
    double dmin2 = 0, dmax2 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ck = sp[k];
        const double below = c.lo[k] - ck, above = ck - c.hi[k];
        const double dmin = below > 0 ? below : (above > 0 ? above : 0.0);
        const double fa = __builtin_fabs(ck - c.lo[k]), fb = __builtin_fabs(ck - c.hi[k]);
        const double dmax = fa < fb ? fb : fa;  // std::max
        dmin2 += dmin * dmin;
        dmax2 += dmax * dmax;
    }
    lb = __builtin_sqrt(dmin2) - sp[3];
    ub = __builtin_sqrt(dmax2) - sp[3];
    return true;
}

// Pass 1: per cell U = min(u0, min_j ub_j) and the number of spheres with lb_j <= U + 1e-6.  A cell of the exterior grid
// whose grown box lies inside the root box counts RM_CAND_NO_LIST.
__global__ __launch_bounds__(kBlock) void cand_count_kernel(RmCandArgs a) {
    const long long cell = static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x / kWave);
    const int lane = threadIdx.x % kWave;
    if (cell >= a.n_cells) return;  // (whole waves: the shuffles below see all 64 lanes)
    CellBox c;
    if (!cell_box(a, cell, c)) return;
    if (a.use_root) {
        bool inside = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) inside = inside && c.lo[k] >= a.root_lo[k] && c.hi[k] <= a.root_hi[k];
        if (inside) {
            if (lane == 0) {
                a.counts[cell] = RM_CAND_NO_LIST;
                a.u[cell] = 0.0;
            }
            return;
        }
    }
    double u = __builtin_inf();
    for (int32_t j = lane; j < c.n; j += kWave) {
        double lb, ub;
        if (cell_bounds(a, c, j, lb, ub)) u = ub < u ? ub : u;
    }
    u = wave_min(u);
    u = u < a.u0 ? u : a.u0;
    uint32_t cnt = 0;
    for (int32_t base = 0; base < c.n; base += kWave) {
        double lb, ub;
        const bool in = cell_bounds(a, c, base + lane, lb, ub) && lb <= u + 1e-6;
        cnt += static_cast<uint32_t>(__popcll(__ballot(in)));
    }
    if (lane == 0) {
        a.counts[cell] = cnt;
        a.u[cell] = u;
    }
}

// Pass 2: the list of every cell that has one (offsets[cell] != RM_CAND_NO_LIST), in increasing sphere order, at its offset
template <typename E>
__global__ __launch_bounds__(kBlock) void cand_fill_kernel(RmCandArgs a, E *list) {
    const long long cell = static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x / kWave);
    const int lane = threadIdx.x % kWave;
    if (cell >= a.n_cells) return;
    const uint32_t off = a.offsets[cell];
    if (off == RM_CAND_NO_LIST) return;
    CellBox c;
    if (!cell_box(a, cell, c)) return;
    const double u = a.u[cell];
    unsigned long long written = off;
    for (int32_t base = 0; base < c.n; base += kWave) {
        double lb, ub;
        const bool in = cell_bounds(a, c, base + lane, lb, ub) && lb <= u + 1e-6;
        const unsigned long long mask = __ballot(in);
        const unsigned long long at = written + static_cast<unsigned>(__popcll(mask & ((1ull << lane) - 1ull)));
        if (in && at < a.list_len) list[at] = static_cast<E>(base + lane);
        written += static_cast<unsigned>(__popcll(mask));
    }
}

// OctBuilder::nearest_prim_box: one wave per node, lanes striding the primitive boxes
__global__ __launch_bounds__(kBlock) void empty_dist_kernel(RmEmptyDistArgs a) {
    const long long node = static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x / kWave);
    const int lane = threadIdx.x % kWave;
    if (node >= a.n_nodes) return;
    float lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = a.boxes[6 * node + k];
        hi[k] = a.boxes[6 * node + 3 + k];
    }
    double best = __builtin_inf();
    for (int32_t i = lane; i < a.n_prims; i += kWave) {
        double g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // box_gap (boundingBox.ts:33-47)
            const float blo = a.prim_lo[3 * static_cast<long long>(i) + k], bhi = a.prim_hi[3 * static_cast<long long>(i) + k];
            g[k] = 0.0;
            if (hi[k] < blo) g[k] = static_cast<double>(blo) - static_cast<double>(hi[k]);
            else if (bhi < lo[k]) g[k] = static_cast<double>(lo[k]) - static_cast<double>(bhi);
        }
        const double d = hypot3_f64(g[0], g[1], g[2]);
        if (d < best) best = d;
    }
    best = wave_min(best);
    if (lane == 0) {
        double r = 0.0;
        if (best != __builtin_inf()) r = best == 0.0 ? 0.0 : (0.0 > best ? 0.0 : best);  // Math.max(0, best), best never -0
        a.out[node] = r;
    }
}

__global__ __launch_bounds__(kBlock) void hypot64_kernel(const double *xyz, int64_t n, double *out) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    out[i] = hypot3_f64(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}

// workgroups for `items` waves; 0 when there is nothing to do or more than a grid dimension holds
unsigned wave_blocks(long long items) {
    if (items <= 0) return 0;
    const long long blocks = (items + kWavesPerBlock - 1) / kWavesPerBlock;
    return blocks > 0x7FFFFFFFll ? 0 : static_cast<unsigned>(blocks);
}

}  // namespace

hipError_t rm_launch_cand_count(const RmCandArgs &a, hipStream_t stream) {
    if (a.n_cells <= 0) return hipSuccess;
    const unsigned blocks = wave_blocks(a.n_cells);
    if (!blocks || !a.grids || !a.spheres || !a.counts || !a.u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cand_count_kernel, dim3(blocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t rm_launch_cand_fill(const RmCandArgs &a, void *list, int elem_bytes, hipStream_t stream) {
    if (a.n_cells <= 0 || a.list_len == 0) return hipSuccess;
    const unsigned blocks = wave_blocks(a.n_cells);
    if (!blocks || !a.grids || !a.spheres || !a.offsets || !a.u || !list || (elem_bytes != 1 && elem_bytes != 2)) return hipErrorInvalidValue;
    if (elem_bytes == 2) hipLaunchKernelGGL(cand_fill_kernel<uint16_t>, dim3(blocks), dim3(kBlock), 0, stream, a, static_cast<uint16_t *>(list));
    else hipLaunchKernelGGL(cand_fill_kernel<uint8_t>, dim3(blocks), dim3(kBlock), 0, stream, a, static_cast<uint8_t *>(list));
    return hipGetLastError();
}

hipError_t rm_launch_empty_dist(const RmEmptyDistArgs &a, hipStream_t stream) {
    if (a.n_nodes <= 0) return hipSuccess;
    const unsigned blocks = wave_blocks(a.n_nodes);
    if (!blocks || !a.boxes || !a.out || a.n_prims < 0 || (a.n_prims > 0 && (!a.prim_lo || !a.prim_hi))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(empty_dist_kernel, dim3(blocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t rm_launch_hypot64(const double *xyz, int64_t n, double *out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(hypot64_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, xyz, n, out);
    return hipGetLastError();
}
