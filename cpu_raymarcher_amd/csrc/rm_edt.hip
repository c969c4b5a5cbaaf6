// rm_edt.hip -- the exact Euclidean distance transform of the points on one side of iso of a lattice of values (gfx950):
// rm_edt_field_device writes, for every point of the set S, the squared index distance to the nearest point of the lattice
// that is not in S.
//
// The rule is the contract of include/rm_raymarch.h ("distances"); tests/edt_model.py restates it in numpy.  The squared
// distance separates: min over (i', j', k') of (i-i')^2 + (j-j')^2 + (k-k')^2 is a minimum along i, then a min-plus with the
// parabola (j-j')^2 along j, then the same along k.  Everything is an integer with one right answer; no floating point
// appears behind the comparison with iso, and no atomic at all.
//   edt_rows_kernel<T>   mapped by point as parts_init_kernel: membership by one wave ballot, the nearest point of T to the
//                        left and to the right within the row from bit scans of the ballot; where a row leaves the wave on
//                        either side the wave walks the row's further 64-point segments until one holds a point of T
//   edt_axis_kernel      one lane per line along j (then along k), adjacent lanes adjacent in i: Meijster's two scans.  The
//                        forward scan builds the lower envelope of the line's parabolas as a stack of (position, break
//                        point, value) in the scratch buffer, slot q of a line where the line's q-th point is in the volume;
//                        the backward scan evaluates the envelope over the line in place
//   edt_reduce_kernel    a grid-stride pass over d2: per workgroup the largest (d2, smallest index) and the points with d2 > 0
//   edt_info_kernel      one workgroup: the partials -> the info
// No thread waits for another, and every loop is bounded by the length of its row or line.  Bounds of the arithmetic: the
// entry refuses lattices with (nu-1)^2 + (nv-1)^2 + (nw-1)^2 > INT32_MAX - 1, so every finite d2 and every partial result is
// below RM_EDT_FAR = INT32_MAX and every index difference is at most 46 340; a sum of two such terms fits unsigned 32 bits.
// RM_EDT_FAR marks an absent parabola: it is skipped, never added to.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_mesh_device.h"

namespace {

constexpr int kFar = INT_MAX;          // RM_EDT_FAR
constexpr unsigned kNoPoint = 1u << 30;  // "no point of T on this side": above every index difference
constexpr unsigned kLineBlock = 64;    // edt_axis_kernel: one wave a workgroup, so that few lines still spread over the CUs
constexpr unsigned kReduceMost = 1024; // edt_reduce_kernel's workgroups at most; edt_info_kernel reads that many partials

// the largest x at which the parabola at i with value gi is not above the one at u > i with value gu:
// floor((u^2 - i^2 + gu - gi) / (2 (u - i))) in 32 bits.  With d = u - i and gu - gi = a * 2d + r, 0 <= r < 2d, it is
// a + floor(((u + i) d + r) / 2d); (u + i) d is (u + i) / 2 times 2d, plus d when u + i is odd.
__host__ __device__ __forceinline__ int edt_sep(int i, int u, int gi, int gu) {
    const int d = u - i, twice = 2 * d, diff = gu - gi;  // gi, gu in [0, INT_MAX): the difference fits
    int a = diff / twice, r = diff - a * twice;
    if (r < 0) {
        r += twice;
        --a;
    }
    const int sum = u + i;
    return a + (sum >> 1) + (((sum & 1) != 0 && r >= d) ? 1 : 0);
}

// the parabola at s with value g, at x
__host__ __device__ __forceinline__ unsigned edt_at(int x, int s, int g) {
    const int d = x - s;
    return static_cast<unsigned>(d * d) + static_cast<unsigned>(g);
}

// a stack entry: the value below, the position and the break point (both below 65 536) above
__host__ __device__ __forceinline__ unsigned long long edt_pack(int s, int t, int g) {
    return (static_cast<unsigned long long>((static_cast<unsigned>(s) << 16) | static_cast<unsigned>(t)) << 32) | static_cast<unsigned>(g);
}

// One line of m points, point u at line[u * stride], in place; stack: m entries, entry q at stack[q * stride].
// Meijster, Roerdink, Hesselink (2000), second phase, over the parabolas that are present.
__host__ __device__ __forceinline__ void edt_line(int *line, unsigned long long *stack, int m, size_t stride) {
    int q = -1, top_s = 0, top_t = 0, top_g = 0;  // the stack's top entry stays in registers
    for (int u = 0; u < m; ++u) {
        const int gu = line[u * stride];
        if (gu == kFar) continue;
        while (q >= 0 && edt_at(top_t, top_s, top_g) > edt_at(top_t, u, gu)) {  // u wins where the top begins to: the top never shows
            if (--q >= 0) {
                const unsigned long long e = stack[q * stride];
                top_s = static_cast<int>(e >> 48);
                top_t = static_cast<int>((e >> 32) & 0xFFFFu);
                top_g = static_cast<int>(e & 0xFFFFFFFFu);
            }
        }
        int w = 0;
        if (q >= 0) {
            w = 1 + edt_sep(top_s, u, top_g, gu);  // above top_t: the top is not above u there
            if (w >= m) continue;
        }
        ++q;
        top_s = u;
        top_t = w;
        top_g = gu;
        stack[q * stride] = edt_pack(u, w, gu);
    }
    if (q < 0) return;  // no parabola: every point of the line stays RM_EDT_FAR
    for (int u = m - 1; u >= 0; --u) {
        line[u * stride] = static_cast<int>(edt_at(u, top_s, top_g));
        if (u == top_t && q > 0) {
            const unsigned long long e = stack[--q * stride];
            top_s = static_cast<int>(e >> 48);
            top_t = static_cast<int>((e >> 32) & 0xFFFFu);
            top_g = static_cast<int>(e & 0xFFFFFFFFu);
        }
    }
}

template <typename T>
__device__ __forceinline__ bool in_set(const RmEdtArgs &a, unsigned l) {
    const double v = static_cast<double>(static_cast<const T *>(a.values)[l]);  // binary32 widens exactly
    return a.outside ? !(v < a.iso) : v < a.iso;
}

// What a lane learns from its wave's ballot `other` of the points of T: the distances to the nearest one before and behind it
// among the lanes of its own row (kNoPoint: none), and whether the row goes on beyond the wave on a side that has none.
// i: the point's index in its row; ahead: the row's points behind it.
struct RowSpan {
    unsigned left, right;
    bool more_left, more_right;
};
__host__ __device__ __forceinline__ RowSpan edt_row_span(unsigned long long other, unsigned lane, unsigned i, unsigned ahead) {
    const unsigned lo = i < lane ? lane - i : 0u, hi = ahead < 63u - lane ? lane + ahead : 63u;  // the row's lanes: lo .. hi
    const unsigned long long upto = (2ull << lane) - 1ull, from = ~((1ull << lane) - 1ull);     // lane 63: 2 << 63 is 0, all bits
    const unsigned long long left_bits = other & upto & ~((1ull << lo) - 1ull), right_bits = other & from & ((2ull << hi) - 1ull);
    RowSpan s = {kNoPoint, kNoPoint, !left_bits && i > lane, !right_bits && ahead > 63u - lane};
    if (left_bits) s.left = lane - (63u - static_cast<unsigned>(__builtin_clzll(left_bits)));
    if (right_bits) s.right = static_cast<unsigned>(__builtin_ctzll(right_bits)) - lane;
    return s;
}

// Wave-uniform: the distance from point base - 1 down to the nearest point of T of the row that starts at `row` < base
// (kNoPoint: none), one 64-point segment a step.  is_t(l): point l is in T.
template <typename IsT>
__device__ __forceinline__ unsigned edt_carry_left(unsigned base, unsigned row, unsigned lane, IsT is_t) {
    for (unsigned end = base;; end -= 64u) {  // the segment end - 64 .. end - 1, not below the row's start
        const bool here = end + lane >= row + 64u;
        const unsigned long long t = __ballot(here && is_t(end - 64u + lane));
        if (t) return static_cast<unsigned>(__builtin_clzll(t)) + (base - end);
        if (end - row <= 64u) return kNoPoint;
    }
}
// the distance from point base + 64 up to the nearest point of T of the row that ends at row_end >= base + 64
template <typename IsT>
__device__ __forceinline__ unsigned edt_carry_right(unsigned base, unsigned row_end, unsigned lane, IsT is_t) {
    for (unsigned start = base + 64u; start <= row_end; start += 64u) {
        const bool here = start + lane <= row_end;
        const unsigned long long t = __ballot(here && is_t(start + lane));
        if (t) return static_cast<unsigned>(__builtin_ctzll(t)) + (start - (base + 64u));
    }
    return kNoPoint;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void edt_rows_kernel(RmEdtArgs a) {
    const unsigned l = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63u, base = l - lane, n = static_cast<unsigned>(a.n);
    const bool valid = l < n;
    const bool in = valid && in_set<T>(a, l);
    const unsigned long long other = __ballot(valid && !in);  // the points of T among the wave's
    const unsigned i = valid ? l % a.nu : 0u;
    RowSpan s = edt_row_span(other, lane, i, a.nu - 1u - i);
    const auto is_t = [&](unsigned at) { return !in_set<T>(a, at); };
    // Only the row of lane 0 can go on before the wave and only the row of lane 63 behind it, so one walk serves every lane.
    const bool more_left = in && s.more_left, more_right = in && s.more_right;
    if (__ballot(more_left)) {
        const unsigned carry = edt_carry_left(base, base - base % a.nu, lane, is_t);
        if (more_left && carry != kNoPoint) s.left = lane + 1u + carry;
    }
    if (__ballot(more_right)) {  // a lane's row goes on behind the wave: the wave's last point is a lattice point
        const unsigned last = base + 63u;
        const unsigned carry = edt_carry_right(base, last - last % a.nu + (a.nu - 1u), lane, is_t);
        if (more_right && carry != kNoPoint) s.right = 64u - lane + carry;
    }
    if (!valid) return;
    const unsigned d = min(s.left, s.right);
    a.d2[l] = !in ? 0 : d == kNoPoint ? kFar : static_cast<int>(d * d);
}

__global__ __launch_bounds__(kLineBlock) void edt_axis_kernel(RmEdtArgs a, unsigned n_lines, unsigned inner, unsigned long long outer, unsigned m,
                                                              unsigned long long stride) {
    const unsigned t = blockIdx.x * kLineBlock + threadIdx.x;
    if (t >= n_lines) return;
    // line t: the points base + u * stride, u < m; lines t and t + 1 are neighbours in i
    const size_t base = static_cast<size_t>(t / inner) * outer + t % inner;
    edt_line(a.d2 + base, a.stack + base, static_cast<int>(m), static_cast<size_t>(stride));
}

// (d2 << 31) | (2^31 - 1 - index): the larger d2 first, then the smaller index; 0: no point of S
struct EdtPartial {
    unsigned long long key, count;
};

// the workgroup's partial in thread 0; `part`: one entry per wave of LDS
__device__ __forceinline__ EdtPartial block_partial(EdtPartial p, EdtPartial *part) {
#pragma unroll
    for (unsigned d = 32; d >= 1; d >>= 1) {
        const unsigned long long k = __shfl_down(p.key, d), c = __shfl_down(p.count, d);
        p.key = k > p.key ? k : p.key;
        p.count += c;
    }
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (unsigned w = 1; w < kWaves; ++w) {
            p.key = part[w].key > p.key ? part[w].key : p.key;
            p.count += part[w].count;
        }
    }
    return p;
}

__global__ __launch_bounds__(kBlock) void edt_reduce_kernel(RmEdtArgs a, EdtPartial *partials) {
    __shared__ EdtPartial s_part[kWaves];
    EdtPartial p = {0ull, 0ull};
    const unsigned n = static_cast<unsigned>(a.n);
    for (unsigned l = blockIdx.x * kBlock + threadIdx.x; l < n; l += gridDim.x * kBlock) {  // n <= 2^30 and the grid's span <= 2^18: no wrap
        const int d = a.d2[l];
        if (d > 0) {
            const unsigned long long key = (static_cast<unsigned long long>(d) << 31) | (0x7FFFFFFFull - l);
            p.key = key > p.key ? key : p.key;
            ++p.count;
        }
    }
    p = block_partial(p, s_part);
    if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

__global__ __launch_bounds__(kBlock) void edt_info_kernel(const EdtPartial *partials, unsigned n_partials, RmEdtInfo *info, long long n) {
    __shared__ EdtPartial s_part[kWaves];
    EdtPartial p = {0ull, 0ull};
    for (unsigned at = threadIdx.x; at < n_partials; at += kBlock) {
        const EdtPartial o = partials[at];
        p.key = o.key > p.key ? o.key : p.key;
        p.count += o.count;
    }
    p = block_partial(p, s_part);
    if (threadIdx.x == 0) {
        info->n_points = n;
        info->n_set = static_cast<long long>(p.count);
        info->max_d2 = static_cast<long long>(p.key >> 31);
        info->argmax = p.count ? static_cast<long long>(0x7FFFFFFFull - (p.key & 0x7FFFFFFFull)) : -1ll;
    }
}

template <typename T>
hipError_t launch_edt(const RmEdtArgs &a, hipStream_t stream, const char **kernel_name) {
    const unsigned n_blocks = static_cast<unsigned>((a.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(edt_rows_kernel<T>, dim3(n_blocks), dim3(kBlock), 0, stream, a);
    if (kernel_name) *kernel_name = "edt_rows_kernel";
    const unsigned long long plane = static_cast<unsigned long long>(a.nu) * a.nv;
    if (a.nv > 1u) {  // along j: line (i, k) starts at k * plane + i
        const unsigned lines = a.nu * a.nw;
        hipLaunchKernelGGL(edt_axis_kernel, dim3((lines + kLineBlock - 1) / kLineBlock), dim3(kLineBlock), 0, stream, a, lines, a.nu, plane, a.nv,
                           static_cast<unsigned long long>(a.nu));
    }
    if (a.nw > 1u) {  // along k: line (i, j) starts at j * nu + i
        const unsigned lines = static_cast<unsigned>(plane);
        hipLaunchKernelGGL(edt_axis_kernel, dim3((lines + kLineBlock - 1) / kLineBlock), dim3(kLineBlock), 0, stream, a, lines, lines, 0ull, a.nw, plane);
    }
    if (kernel_name && (a.nv > 1u || a.nw > 1u)) *kernel_name = "edt_axis_kernel";
    const unsigned groups = n_blocks < kReduceMost ? n_blocks : kReduceMost;
    EdtPartial *partials = static_cast<EdtPartial *>(a.partials);
    hipLaunchKernelGGL(edt_reduce_kernel, dim3(groups), dim3(kBlock), 0, stream, a, partials);
    hipLaunchKernelGGL(edt_info_kernel, dim3(1), dim3(kBlock), 0, stream, partials, groups, a.info, a.n);
    return hipGetLastError();
}

}  // namespace

static_assert(sizeof(EdtPartial) * kReduceMost == RM_EDT_PARTIAL_BYTES, "the entries reserve this much for the partials");

hipError_t rm_launch_edt_field(const RmEdtArgs &a, hipStream_t stream, const char **kernel_name) {
    if (a.n <= 0 || a.n > (1ll << 30) || static_cast<long long>(a.nu) * a.nv * a.nw != a.n) return hipErrorInvalidValue;
    const long long u = a.nu - 1ll, v = a.nv - 1ll, w = a.nw - 1ll;
    if (u * u + v * v + w * w > INT_MAX - 1ll) return hipErrorInvalidValue;
    return a.f32 ? launch_edt<float>(a, stream, kernel_name) : launch_edt<double>(a, stream, kernel_name);
}
