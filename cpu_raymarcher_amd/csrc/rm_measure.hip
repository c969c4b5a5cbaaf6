// rm_measure.hip -- how much there is of a solid on a lattice (gfx950): rm_measure_field_device over a dense volume and
// rm_measure_tiles_device over the 9 x 9 x 9 tiles of the kept blocks plus closed forms for the dropped ones.
//
// The rule is the contract of include/rm_raymarch.h ("measures"); tests/measure_model.py restates it in numpy.  Every quantity
// is an integer -- counts of inside points, sums of their indices and index products, counts of lattice edges whose ends differ
// in `inside`, and an index box --, so a sum does not depend on its order and nothing here is ordered: each workgroup reduces
// its lanes' sums (shuffles within a wave, LDS across the four waves) into ONE partial record in the caller's scratch, and one
// last workgroup adds the partials up.  No atomics, nothing to zero beforehand, one global write per workgroup.
//   measure_field_kernel<T>   a persistent grid of waves, each over whole lattice rows: a lane takes i = lane, lane + 64, ...
//   measure_tiles_kernel      per kept block: the tile staged in LDS, the block's owned points and edges, local indices
//   measure_blocks_kernel     one lane per block: the closed forms of a dropped block that lies inside
//   measure_final_kernel      the partials -> the rm_measure record
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_kernels.h"

namespace {

constexpr unsigned kBlock = RM_MESH_BLOCK, kWaves = kBlock / 64;  // the meshers' workgroup
constexpr unsigned kTile = RM_SPARSE_TILE, kB = RM_SPARSE_BLOCK;

// the sums of a partial record, in RmMeasurePartial::sum's order
enum { S_INSIDE, S_NONFINITE, S_I, S_J, S_K, S_II, S_JJ, S_KK, S_IJ, S_JK, S_KI, S_CROSS_I, S_CROSS_J, S_CROSS_K, S_BLOCKS_INSIDE, S_COUNT };
static_assert(S_COUNT == RM_MEASURE_SUMS, "RmMeasurePartial::sum");

struct Box {
    int lo[3], hi[3];
    __device__ void clear() {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = INT_MAX;
            hi[c] = -1;
        }
    }
    __device__ void take(int c, int low, int high) {
        lo[c] = min(lo[c], low);
        hi[c] = max(hi[c], high);
    }
};

// The sums and the boxes of the workgroup's 256 lanes -> thread 0 (the other threads' values mean nothing afterwards).
// `s_sum`: kWaves x N values of LDS, `s_box`: kWaves x 6 words.  The caller owns the barrier ahead of a second use.
template <typename T, int N>
__device__ __forceinline__ void block_reduce(T (&sum)[N], Box &box, T *s_sum, int *s_box) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (unsigned d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int n = 0; n < N; ++n) sum[n] += __shfl_down(sum[n], d);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            box.lo[c] = min(box.lo[c], __shfl_down(box.lo[c], d));
            box.hi[c] = max(box.hi[c], __shfl_down(box.hi[c], d));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) s_sum[wave * N + n] = sum[n];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s_box[wave * 6 + c] = box.lo[c];
            s_box[wave * 6 + 3 + c] = box.hi[c];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (unsigned w = 1; w < kWaves; ++w) {
#pragma unroll
            for (int n = 0; n < N; ++n) sum[n] += s_sum[w * N + n];
#pragma unroll
            for (int c = 0; c < 3; ++c) box.take(c, s_box[w * 6 + c], s_box[w * 6 + 3 + c]);
        }
    }
}

__device__ __forceinline__ void store_partial(RmMeasurePartial *out, const long long (&sum)[S_COUNT], const Box &box) {
#pragma unroll
    for (int n = 0; n < S_COUNT; ++n) out->sum[n] = sum[n];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out->lo[c] = box.lo[c];
        out->hi[c] = box.hi[c];
    }
}

// ---- the dense volume: a wave per row, the rows dealt round-robin to the grid's waves.  What the kernel waits for is the
// latency of its loads, not their number: two chunks of 64 points a step keep all eight loads in flight, and the grid is exactly
// what the device holds at a time, so no workgroup waits for a second round.

// the product of two 32-bit factors in 64 bits
__device__ __forceinline__ long long wide(unsigned x, unsigned y) { return static_cast<long long>(static_cast<unsigned long long>(x) * y); }

template <typename T>
__global__ __launch_bounds__(kBlock) void measure_field_kernel(RmMeasureFieldArgs a) {
    __shared__ long long s_sum[kWaves * S_COUNT];
    __shared__ int s_box[kWaves * 6];
    const T *values = static_cast<const T *>(a.values);
    const unsigned lane = threadIdx.x & 63u;
    const unsigned rows = a.nv * a.nw;  // at most 2^30 points: rows, and every linear index below, fit 32 bits
    const unsigned plane = a.nu * a.nv;
    long long sum[S_COUNT];
#pragma unroll
    for (int n = 0; n < S_COUNT; ++n) sum[n] = 0;
    Box box;
    box.clear();
    // The wave's rows: first, first + step, ...; (j, k) follow by addition.  The wave's number is made a scalar, so the row, its
    // (j, k) and its base address are, and a load is a scalar base plus the lane's i.
    const unsigned step = gridDim.x * kWaves, step_k = step / a.nv, step_j = step - step_k * a.nv;
    unsigned row = blockIdx.x * kWaves + static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    unsigned k = row / a.nv, j = row - k * a.nv;
    for (; row < rows; row += step) {
        const bool more_j = j + 1u < a.nv, more_k = k + 1u < a.nw;
        const T *at = values + static_cast<size_t>(row) * a.nu;
        // this row's share of the lane: the count, the sum of i and of i * i; j and k are the row's and join at its end
        unsigned count = 0, sum_i = 0, non_finite = 0, cross_i = 0, cross_j = 0, cross_k = 0;
        unsigned long long sum_ii = 0;
        int lo_i = INT_MAX, hi_i = -1;
        // Two chunks of 64 points a step, every load unconditional -- an index beyond the row's end, or a neighbour that does
        // not exist, reads the point itself or the row's last point instead and is not counted --, so that the eight loads of
        // a step are in flight together.
        const T *at_j = at + (more_j ? a.nu : 0u), *at_k = at + (more_k ? plane : 0u);
        const unsigned last = a.nu - 1u;
        for (unsigned first = 0; first < a.nu; first += 128u) {
            double v[2], vi[2], vj[2], vk[2];
            unsigned i[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                i[h] = first + 64u * h + lane;
                const unsigned here = min(i[h], last);
                v[h] = static_cast<double>(at[here]);
                vi[h] = static_cast<double>(at[min(i[h] + 1u, last)]);
                vj[h] = static_cast<double>(at_j[here]);
                vk[h] = static_cast<double>(at_k[here]);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool valid = i[h] < a.nu, in = valid && v[h] < a.iso;
                non_finite += valid && !isfinite(v[h]) ? 1u : 0u;
                cross_i += i[h] < last && (vi[h] < a.iso) != in ? 1u : 0u;
                cross_j += valid && more_j && (vj[h] < a.iso) != in ? 1u : 0u;
                cross_k += valid && more_k && (vk[h] < a.iso) != in ? 1u : 0u;
                if (in) {
                    ++count;
                    sum_i += i[h];  // at most 1 024 indices below 2^16 per lane and row: below 2^26
                    sum_ii += static_cast<unsigned long long>(i[h]) * i[h];
                    lo_i = min(lo_i, static_cast<int>(i[h]));
                    hi_i = static_cast<int>(i[h]);  // i only grows
                }
            }
        }
        // j, k < 2^16 and count <= 2^10: j * count, k * count and j * j fit 32 bits, and every product below is one of two
        // 32-bit factors, formed in 64 bits
        const unsigned jc = j * count, kc = k * count;
        sum[S_INSIDE] += count;
        sum[S_NONFINITE] += non_finite;
        sum[S_I] += sum_i;
        sum[S_J] += jc;
        sum[S_K] += kc;
        sum[S_II] += static_cast<long long>(sum_ii);
        sum[S_JJ] += wide(j * j, count);
        sum[S_KK] += wide(k * k, count);
        sum[S_IJ] += wide(j, sum_i);
        sum[S_JK] += wide(jc, k);
        sum[S_KI] += wide(k, sum_i);
        sum[S_CROSS_I] += cross_i;
        sum[S_CROSS_J] += cross_j;
        sum[S_CROSS_K] += cross_k;
        if (count) {
            box.take(0, lo_i, hi_i);
            box.take(1, static_cast<int>(j), static_cast<int>(j));
            box.take(2, static_cast<int>(k), static_cast<int>(k));
        }
        j += step_j;
        k += step_k;
        if (j >= a.nv) {
            j -= a.nv;
            ++k;
        }
    }
    block_reduce(sum, box, s_sum, s_box);
    if (threadIdx.x == 0) store_partial(a.partials + blockIdx.x, sum, box);
}

// ---- the kept blocks

// how many points of an axis with n points and nb blocks block b owns: 8, and the last block the rest (9 when 8 nb = n - 1)
__device__ __forceinline__ unsigned owned_on_axis(unsigned n, unsigned nb, unsigned b) { return b + 1u == nb ? n - kB * b : kB; }

__global__ __launch_bounds__(kBlock) void measure_tiles_kernel(RmMeasureTilesArgs a) {
    __shared__ double s_tile[kTile];
    __shared__ unsigned s_sum[kWaves * S_COUNT];
    __shared__ int s_box[kWaves * 6];
    const unsigned r = blockIdx.x;
    const double *src = a.tiles + static_cast<size_t>(r) * kTile;
    for (unsigned t = threadIdx.x; t < kTile; t += kBlock) s_tile[t] = src[t];
    __syncthreads();
    // the block of slot r; a list entry outside the lattice owns nothing
    const unsigned b = static_cast<unsigned>(a.list[r]);
    const unsigned row = b / a.nbu, bx = b - row * a.nbu, bz = row / a.nbv, by = row - bz * a.nbv;
    const bool in_lattice = bz < a.nbw;
    const unsigned ox = in_lattice ? owned_on_axis(a.nu, a.nbu, bx) : 0u, oy = in_lattice ? owned_on_axis(a.nv, a.nbv, by) : 0u,
                   oz = in_lattice ? owned_on_axis(a.nw, a.nbw, bz) : 0u;
    const unsigned X = kB * bx, Y = kB * by, Z = kB * bz;
    // local sums: 729 points with local indices up to 8 stay far below 2^32
    unsigned sum[S_COUNT];
#pragma unroll
    for (int n = 0; n < S_COUNT; ++n) sum[n] = 0;
    Box box;
    box.clear();
#pragma unroll
    for (unsigned h = 0; h < 3; ++h) {
        const unsigned p = threadIdx.x + h * kBlock;
        const unsigned x = p % 9u, y = (p / 9u) % 9u, z = p / 81u;
        if (!(p < kTile && x < ox && y < oy && z < oz)) continue;
        const double v = s_tile[p];
        const bool in = v < a.iso;
        sum[S_NONFINITE] += isfinite(v) ? 0u : 1u;
        // an edge exists when its high end is a lattice point: by index, whatever the tile holds beyond the lattice
        if (X + x + 1u < a.nu) sum[S_CROSS_I] += (s_tile[p + 1u] < a.iso) != in ? 1u : 0u;
        if (Y + y + 1u < a.nv) sum[S_CROSS_J] += (s_tile[p + 9u] < a.iso) != in ? 1u : 0u;
        if (Z + z + 1u < a.nw) sum[S_CROSS_K] += (s_tile[p + 81u] < a.iso) != in ? 1u : 0u;
        if (in) {
            sum[S_INSIDE] += 1u;
            sum[S_I] += x;
            sum[S_J] += y;
            sum[S_K] += z;
            sum[S_II] += x * x;
            sum[S_JJ] += y * y;
            sum[S_KK] += z * z;
            sum[S_IJ] += x * y;
            sum[S_JK] += y * z;
            sum[S_KI] += z * x;
            box.take(0, static_cast<int>(x), static_cast<int>(x));
            box.take(1, static_cast<int>(y), static_cast<int>(y));
            box.take(2, static_cast<int>(z), static_cast<int>(z));
        }
    }
    block_reduce(sum, box, s_sum, s_box);
    if (threadIdx.x != 0) return;
    // the base indices join once per workgroup: sum of (X + x) = X n + sum x, of (X + x)(Y + y) = X Y n + X sum y + Y sum x + sum x y
    const long long n = sum[S_INSIDE], lx = X, ly = Y, lz = Z, sx = sum[S_I], sy = sum[S_J], sz = sum[S_K];
    long long total[S_COUNT];
    total[S_INSIDE] = n;
    total[S_NONFINITE] = sum[S_NONFINITE];
    total[S_I] = lx * n + sx;
    total[S_J] = ly * n + sy;
    total[S_K] = lz * n + sz;
    total[S_II] = lx * lx * n + 2 * lx * sx + sum[S_II];
    total[S_JJ] = ly * ly * n + 2 * ly * sy + sum[S_JJ];
    total[S_KK] = lz * lz * n + 2 * lz * sz + sum[S_KK];
    total[S_IJ] = lx * ly * n + lx * sy + ly * sx + sum[S_IJ];
    total[S_JK] = ly * lz * n + ly * sz + lz * sy + sum[S_JK];
    total[S_KI] = lz * lx * n + lz * sx + lx * sz + sum[S_KI];
    total[S_CROSS_I] = sum[S_CROSS_I];
    total[S_CROSS_J] = sum[S_CROSS_J];
    total[S_CROSS_K] = sum[S_CROSS_K];
    total[S_BLOCKS_INSIDE] = 0;
    if (n) {
        const int base[3] = {static_cast<int>(X), static_cast<int>(Y), static_cast<int>(Z)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            box.lo[c] += base[c];
            box.hi[c] += base[c];
        }
    }
    store_partial(a.partials + r, total, box);
}

// ---- the dropped blocks: every owned point of a block with d - iso < 0 is inside

// the sum of i and of i * i over i = first .. first + count - 1
__device__ __forceinline__ void range_sums(long long first, long long count, long long *s1, long long *s2) {
    *s1 = count * first + count * (count - 1) / 2;
    *s2 = count * first * first + first * count * (count - 1) + (count - 1) * count * (2 * count - 1) / 6;
}

__global__ __launch_bounds__(kBlock) void measure_blocks_kernel(RmMeasureTilesArgs a) {
    __shared__ long long s_sum[kWaves * S_COUNT];
    __shared__ int s_box[kWaves * 6];
    long long sum[S_COUNT];
#pragma unroll
    for (int n = 0; n < S_COUNT; ++n) sum[n] = 0;
    Box box;
    box.clear();
    for (unsigned b = blockIdx.x * kBlock + threadIdx.x; b < a.n_blocks; b += gridDim.x * kBlock) {
        if (!(a.slot[b] < 0 && a.dist[b] - a.iso < 0.0)) continue;
        const unsigned row = b / a.nbu, bx = b - row * a.nbu, bz = row / a.nbv, by = row - bz * a.nbv;
        const long long first[3] = {kB * bx, kB * by, kB * bz};
        const long long count[3] = {owned_on_axis(a.nu, a.nbu, bx), owned_on_axis(a.nv, a.nbv, by), owned_on_axis(a.nw, a.nbw, bz)};
        long long s1[3], s2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            range_sums(first[c], count[c], &s1[c], &s2[c]);
            box.take(c, static_cast<int>(first[c]), static_cast<int>(first[c] + count[c] - 1));
        }
        sum[S_INSIDE] += count[0] * count[1] * count[2];
        sum[S_I] += s1[0] * count[1] * count[2];
        sum[S_J] += s1[1] * count[2] * count[0];
        sum[S_K] += s1[2] * count[0] * count[1];
        sum[S_II] += s2[0] * count[1] * count[2];
        sum[S_JJ] += s2[1] * count[2] * count[0];
        sum[S_KK] += s2[2] * count[0] * count[1];
        sum[S_IJ] += s1[0] * s1[1] * count[2];
        sum[S_JK] += s1[1] * s1[2] * count[0];
        sum[S_KI] += s1[2] * s1[0] * count[1];
        sum[S_BLOCKS_INSIDE] += 1;
    }
    block_reduce(sum, box, s_sum, s_box);
    if (threadIdx.x == 0) store_partial(a.partials + a.n_kept + blockIdx.x, sum, box);
}

// ---- the partials -> the record.  One workgroup; n_partials may be 0 (a lattice without points): zero sums, the empty box.

__global__ __launch_bounds__(kBlock) void measure_final_kernel(const RmMeasurePartial *partials, unsigned n_partials, RmMeasure *out, long long n_points,
                                                               long long n_blocks, long long n_kept) {
    __shared__ long long s_sum[kWaves * S_COUNT];
    __shared__ int s_box[kWaves * 6];
    long long sum[S_COUNT];
#pragma unroll
    for (int n = 0; n < S_COUNT; ++n) sum[n] = 0;
    Box box;
    box.clear();
    for (unsigned at = threadIdx.x; at < n_partials; at += kBlock) {
        const RmMeasurePartial *p = partials + at;
#pragma unroll
        for (int n = 0; n < S_COUNT; ++n) sum[n] += p->sum[n];
#pragma unroll
        for (int c = 0; c < 3; ++c) box.take(c, p->lo[c], p->hi[c]);
    }
    block_reduce(sum, box, s_sum, s_box);
    if (threadIdx.x != 0) return;
    out->n_points = n_points;
    out->n_inside = sum[S_INSIDE];
    out->n_nonfinite = sum[S_NONFINITE];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out->sum1[c] = sum[S_I + c];
        out->crossings[c] = sum[S_CROSS_I + c];
        out->lo[c] = box.lo[c];
        out->hi[c] = box.hi[c];
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) out->sum2[c] = sum[S_II + c];
    out->n_blocks = n_blocks;
    out->n_kept = n_kept;
    out->n_blocks_inside = sum[S_BLOCKS_INSIDE];
    out->reserved = 0;
}

// a persistent grid: per_cu workgroups a CU at most, and no more than there is work
unsigned persistent_grid(size_t items, int num_cus, unsigned per_cu) {
    const size_t most = static_cast<size_t>(per_cu) * static_cast<size_t>(num_cus > 0 ? num_cus : 256);
    return static_cast<unsigned>(items < most ? (items ? items : 1) : most);
}

// the workgroups of measure_field_kernel a CU holds at a time (asked of the runtime once, for the device that is current: the
// entries set their context's device first): a larger grid would run in rounds
unsigned field_groups_per_cu() {
    static const unsigned per_cu = [] {
        int d = 0, f = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&d, measure_field_kernel<double>, kBlock, 0) != hipSuccess) d = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&f, measure_field_kernel<float>, kBlock, 0) != hipSuccess) f = 0;
        const int both = d < f ? d : f;
        return static_cast<unsigned>(both >= 1 && both <= 8 ? both : 4);
    }();
    return per_cu;
}

}  // namespace

unsigned int rm_measure_field_groups(long long n, unsigned int nv, unsigned int nw, int num_cus) {
    return n > 0 ? persistent_grid((static_cast<size_t>(nv) * nw + kWaves - 1) / kWaves, num_cus, field_groups_per_cu()) : 0u;
}

unsigned int rm_measure_block_groups(unsigned int n_blocks, int num_cus) { return persistent_grid((n_blocks + kBlock - 1) / kBlock, num_cus, 8u); }

hipError_t rm_launch_measure_field(const RmMeasureFieldArgs &a, unsigned int n_groups, hipStream_t stream, const char **kernel_name) {
    if (a.n < 0 || a.n > (1ll << 30) || (a.n > 0) != (n_groups > 0)) return hipErrorInvalidValue;
    if (a.n > 0) {
        if (a.f32) {
            if (kernel_name) *kernel_name = "measure_field_kernel<float>";
            hipLaunchKernelGGL(measure_field_kernel<float>, dim3(n_groups), dim3(kBlock), 0, stream, a);
        } else {
            if (kernel_name) *kernel_name = "measure_field_kernel<double>";
            hipLaunchKernelGGL(measure_field_kernel<double>, dim3(n_groups), dim3(kBlock), 0, stream, a);
        }
    } else if (kernel_name) {
        *kernel_name = "measure_final_kernel";
    }
    hipLaunchKernelGGL(measure_final_kernel, dim3(1), dim3(kBlock), 0, stream, a.partials, n_groups, a.out, a.n, 0ll, 0ll);
    return hipGetLastError();
}

hipError_t rm_launch_measure_tiles(const RmMeasureTilesArgs &a, unsigned int n_groups, hipStream_t stream, const char **kernel_name) {
    if (a.n_blocks == 0 || a.n_blocks > RM_SPARSE_MAX_BLOCKS || a.n_kept > a.n_blocks || n_groups == 0) return hipErrorInvalidValue;
    if (kernel_name) *kernel_name = a.n_kept ? "measure_tiles_kernel" : "measure_blocks_kernel";
    if (a.n_kept) hipLaunchKernelGGL(measure_tiles_kernel, dim3(a.n_kept), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(measure_blocks_kernel, dim3(n_groups), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(measure_final_kernel, dim3(1), dim3(kBlock), 0, stream, a.partials, a.n_kept + n_groups, a.out, a.n, static_cast<long long>(a.n_blocks),
                       static_cast<long long>(a.n_kept));
    return hipGetLastError();
}
