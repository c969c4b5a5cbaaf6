// rm_frame_ops.hip -- rank 0's side of the row-tile shard (gfx950): ONE kernel that puts the gathered stripes of
// every rank at their place in the row-major frame and combines the ranks' partial diagnostics.
//
// Replaces the fan-in of the reference's main thread: `depthBuffer.set(tile, yStart * width)` per worker result
// (src/main.ts:461-468) and, for the diagnostics (src/main.ts:528-548: a sum, a max and a min, which combine
// exactly from per-rank partial results), the single pass over the gathered counters.  HBM-bound byte movement:
// 16-byte loads and stores, one workgroup per (stripe, column chunk); no reshaping into anything else.
#include <hip/hip_runtime.h>

#include "rm_device.h"
#include "rm_kernels.h"

namespace {

// stripe_src[s] = (rank << 16) | local stripe index of frame stripe s within that rank's packed rows
__global__ __launch_bounds__(256) void assemble_kernel(const unsigned char *__restrict__ gathered, long long rank_stride,
                                                       long long section_offset, int row_bytes, int height, int stripe_rows,
                                                       const int *__restrict__ stripe_src, int n_stripes,
                                                       unsigned char *__restrict__ frame, long long acc_offset, int world,
                                                       RmDiagDevice *acc, int chunks_per_stripe) {
    const int s = blockIdx.x / chunks_per_stripe, chunk = blockIdx.x - s * chunks_per_stripe;
    if (s < n_stripes) {
        const int src = stripe_src[s];
        const int rank = src >> 16, local = src & 0xFFFF;
        const int y0 = s * stripe_rows;
        const int rows = min(stripe_rows, height - y0);
        const long long bytes = static_cast<long long>(rows) * row_bytes;  // a stripe is contiguous on both sides
        const unsigned char *from = gathered + rank * rank_stride + section_offset + static_cast<long long>(local) * stripe_rows * row_bytes;
        unsigned char *to = frame + static_cast<long long>(y0) * row_bytes;
        if (((reinterpret_cast<uintptr_t>(from) | reinterpret_cast<uintptr_t>(to) | static_cast<uintptr_t>(bytes)) & 15) == 0) {
            const long long n16 = bytes >> 4;
            const uint4 *f4 = reinterpret_cast<const uint4 *>(from);
            uint4 *t4 = reinterpret_cast<uint4 *>(to);
            const long long step = static_cast<long long>(chunks_per_stripe) * 256;
            long long i = static_cast<long long>(chunk) * 256 + threadIdx.x;
            for (; i + 3 * step < n16; i += 4 * step) {  // four 16-B loads in flight per lane
                const uint4 a = f4[i], b = f4[i + step], c = f4[i + 2 * step], d = f4[i + 3 * step];
                t4[i] = a;
                t4[i + step] = b;
                t4[i + 2 * step] = c;
                t4[i + 3 * step] = d;
            }
            for (; i < n16; i += step) t4[i] = f4[i];
        } else {
            for (long long i = static_cast<long long>(chunk) * 256 + threadIdx.x; i < bytes; i += static_cast<long long>(chunks_per_stripe) * 256)
                to[i] = from[i];
        }
    }
    // combined diagnostics: sums add, max of max, min of min (a rank without rows holds the neutral elements)
    if (blockIdx.x == 0 && threadIdx.x == 0 && acc && acc_offset >= 0) {
        unsigned long long ts = 0, ti = 0;
        unsigned int mx = 0, mn = 0xFFFFFFFFu;
        for (int r = 0; r < world; ++r) {
            const RmDiagDevice *p = reinterpret_cast<const RmDiagDevice *>(gathered + r * rank_stride + acc_offset);
            ts += p->total_sdf;
            ti += p->total_iters;
            mx = p->max_sdf > mx ? p->max_sdf : mx;
            mn = p->min_sdf < mn ? p->min_sdf : mn;
        }
        acc->total_sdf = ts;
        acc->total_iters = ti;
        acc->max_sdf = mx;
        acc->min_sdf = mn;
        acc->pad = 0;
    }
}


// ------------------------------------------------------------------ compare_kernel (rm_compare_frames_device)
//
// Two G-buffer sets of the same frames, B against A: the difference image of one of the four buffers (or of the G-buffer's
// surface mask) and a 128-byte record of exact integer statistics per frame.  A per-pixel integer function plus a reduction:
// HBM-bound (16 B read, 4 B written per pixel), so the shape is that of assemble_kernel and reduce_kernel --
//   * blockIdx.y is the frame, blockIdx.x a share of its pixels; one launch for the whole batch;
//   * a lane takes GROUPS of 16 consecutive pixels: 16 B of depth, 48 B of normal, 32 B of each counter per side -- sixteen
//     16-byte loads in flight per lane -- and 64 B of image, stored as four 16-byte values;
//   * frame k starts at element k * N of every buffer, so its slices are aligned differently per frame and per buffer.  The
//     groups start `head` pixels into the frame (0 .. 15, the value that 16-byte aligns the most bytes per pixel: with
//     16-byte aligned bases ALL slices, whatever k * N is); a slice that is still misaligned is read element by element into
//     the same registers (the flags are the same for the whole workgroup: scalar branches).  The head and the tail behind the
//     last whole group (at most 30 pixels) are taken one pixel per lane by the frame's first workgroup;
//   * MAP and STATS are template parameters: they decide what is computed per pixel (and which buffers are read at all).
//     An absent pair is a workgroup-uniform branch around its loads; its registers then hold a value that is equal on both
//     sides and no surface ((128,128,128) for the normal), so every field derived from it comes out 0 without a test;
//   * statistics: per lane in registers (sums of a group in 32 bits, folded into 64 bits per group), per wave by __shfl_down,
//     per workgroup in LDS.  A frame of one workgroup writes its record directly.  Otherwise the workgroup's first lane
//     stores the 16 words of a partial record of its own (write-through stores, nothing shared, no atomics on data), waits for
//     them and takes a ticket from the frame's counter; the workgroup whose ticket is the last one acquires, adds up the
//     frame's partial records with all its lanes, writes the record and leaves the counter at zero for its next user.
//     Partial records are overwritten whole by their next user: nothing to clear.  All results are exact integers, so the
//     order of summation does not matter.
// A lane counts pixels in 32 bits: it sees at most N / (256 * workgroups of the frame) + 30 of them.

constexpr int CMP_WORDS = 16, CMP_SUMS = 14;  // words [0, 14) of a partial record add, [14, 16) take the maximum
enum { W_SDF_A, W_SDF_B, W_ITERS_A, W_ITERS_B, W_ABS_DEPTH, W_SURF_A, W_SURF_B, W_ONLY_A, W_ONLY_B, W_DEPTH_DIFF, W_NORMAL_DIFF,
       W_COUNTERS_DIFF, W_B_CHEAPER, W_A_CHEAPER, W_MAX_DEPTH, W_MAX_NORMAL };

struct CmpAcc {
    unsigned long long sum[5];  // W_SDF_A .. W_ABS_DEPTH
    unsigned int group[5];      // the same, of the group in hand
    unsigned int cnt[9];        // W_SURF_A .. W_A_CHEAPER
    unsigned int mx[2];
};

__device__ __forceinline__ unsigned int absdiff(unsigned int a, unsigned int b) { return a > b ? a - b : b - a; }

// One pixel: the normals as 24 bits (R lowest), everything else as the stored value.  Returns the image's uchar4 as a word.
template <int MAP, bool STATS>
__device__ __forceinline__ unsigned int compare_pixel(CmpAcc &c, unsigned int da, unsigned int db, unsigned int na, unsigned int nb,
                                                      unsigned int sa, unsigned int sb, unsigned int ia, unsigned int ib, unsigned int gain) {
    const bool surf_a = na != 0x808080u, surf_b = nb != 0x808080u;  // raymarcher.ts:97-105
    unsigned int dn = 0;
    if (STATS || MAP == RM_CMP_NORMAL) {
        dn = absdiff(na & 255u, nb & 255u);
        const unsigned int g = absdiff((na >> 8) & 255u, (nb >> 8) & 255u), b = absdiff(na >> 16, nb >> 16);
        dn = g > dn ? g : dn;
        dn = b > dn ? b : dn;
    }
    if (STATS) {
        const unsigned int dd = absdiff(da, db);
        c.group[W_SDF_A] += sa;
        c.group[W_SDF_B] += sb;
        c.group[W_ITERS_A] += ia;
        c.group[W_ITERS_B] += ib;
        c.group[W_ABS_DEPTH] += dd;
        c.cnt[W_SURF_A - W_SURF_A] += surf_a;
        c.cnt[W_SURF_B - W_SURF_A] += surf_b;
        c.cnt[W_ONLY_A - W_SURF_A] += surf_a && !surf_b;
        c.cnt[W_ONLY_B - W_SURF_A] += surf_b && !surf_a;
        c.cnt[W_DEPTH_DIFF - W_SURF_A] += da != db;
        c.cnt[W_NORMAL_DIFF - W_SURF_A] += na != nb;
        c.cnt[W_COUNTERS_DIFF - W_SURF_A] += sa != sb || ia != ib;
        c.cnt[W_B_CHEAPER - W_SURF_A] += sb < sa;
        c.cnt[W_A_CHEAPER - W_SURF_A] += sa < sb;
        c.mx[0] = dd > c.mx[0] ? dd : c.mx[0];
        c.mx[1] = dn > c.mx[1] ? dn : c.mx[1];
    }
    if (MAP == RM_CMP_NONE) return 0u;
    if (MAP == RM_CMP_SURFACE) return 0xFF000000u | (surf_a && surf_b ? 0x606060u : surf_b ? 0xFFu : surf_a ? 0xFF00u : 0u);
    if (MAP == RM_CMP_NORMAL) {
        const unsigned int m = min(dn * gain, 255u);
        return 0xFF000000u | m | (m << 8);
    }
    const unsigned int a = MAP == RM_CMP_SDF ? sa : MAP == RM_CMP_ITERS ? ia : da, b = MAP == RM_CMP_SDF ? sb : MAP == RM_CMP_ITERS ? ib : db;
    const unsigned int m = min(absdiff(a, b) * gain, 255u);  // (65535 * 255 fits)
    return 0xFF000000u | (b > a ? m : m << 8);               // red: B has or costs more; green: A; equal: m is 0
}

__device__ __forceinline__ void fold_group(CmpAcc &c) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        c.sum[k] += c.group[k];
        c.group[k] = 0;
    }
}

// NW words of one lane's share of a group: 16-byte loads, or element loads (E: the buffer's element type) into the same words
template <int NW, typename E>
__device__ __forceinline__ void load_group(const E *p, bool present, bool vec, unsigned int fill, unsigned int (&w)[NW]) {
    if (!present) {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = fill;
    } else if (vec) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int k = 0; k < NW / 4; ++k) {
            const uint4 v = q[k];
            w[4 * k] = v.x;
            w[4 * k + 1] = v.y;
            w[4 * k + 2] = v.z;
            w[4 * k + 3] = v.w;
        }
    } else {
        constexpr int PER = 4 / static_cast<int>(sizeof(E));
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            unsigned int x = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) x |= static_cast<unsigned int>(p[k * PER + j]) << (8 * static_cast<int>(sizeof(E)) * j);
            w[k] = x;
        }
    }
}

// the 24 bits of pixel P (a constant after unrolling) of a group's 48 normal bytes
template <int P>
__device__ __forceinline__ unsigned int normal_of(const unsigned int (&w)[12]) {
    constexpr int J = (3 * P) >> 2, SH = (3 * P) & 3;
    if (SH <= 1) return (w[J] >> (8 * SH)) & 0xFFFFFFu;
    return __builtin_amdgcn_alignbyte(w[J + 1 < 12 ? J + 1 : J], w[J], SH) & 0xFFFFFFu;  // (SH >= 2 never meets J == 11)
}

__device__ __forceinline__ void store_pixel(uint8_t *rgba, long long i, unsigned int px, bool whole) {
    if (whole) {
        reinterpret_cast<unsigned int *>(rgba)[i] = px;  // a whole uchar4
    } else {  // an image that does not start on a 4-byte boundary
#pragma unroll
        for (int k = 0; k < 4; ++k) rgba[4 * i + k] = static_cast<uint8_t>(px >> (8 * k));
    }
}

// sums and maxima of the workgroup's lanes -> v of thread 0
__device__ __forceinline__ void cmp_combine(unsigned long long (&v)[CMP_WORDS], const unsigned long long (&o)[CMP_WORDS]) {
#pragma unroll
    for (int k = 0; k < CMP_WORDS; ++k) v[k] = k < CMP_SUMS ? v[k] + o[k] : (o[k] > v[k] ? o[k] : v[k]);
}
__device__ __forceinline__ void cmp_block_reduce(unsigned long long (&v)[CMP_WORDS]) {
    __shared__ unsigned long long sh[4][CMP_WORDS];
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o[CMP_WORDS];
#pragma unroll
        for (int k = 0; k < CMP_WORDS; ++k) o[k] = __shfl_down(v[k], off);
        cmp_combine(v, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < CMP_WORDS; ++k) sh[w][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < 4; ++j) cmp_combine(v, sh[j]);
    }
    __syncthreads();  // (sh is written again when the frame's last workgroup adds up the partial records)
}

__device__ __forceinline__ void cmp_write_record(RmCompareStats *out, long long npx, const unsigned long long (&v)[CMP_WORDS]) {
    out->pixels = static_cast<unsigned long long>(npx);
#pragma unroll
    for (int k = 0; k < CMP_SUMS; ++k) out->sums[k] = v[k];
    out->max_abs_depth = static_cast<unsigned int>(v[W_MAX_DEPTH]);
    out->max_abs_normal = static_cast<unsigned int>(v[W_MAX_NORMAL]);
}

template <int MAP, bool STATS>
__global__ __launch_bounds__(256) void compare_kernel(const RmCompareArgs A) {
    constexpr bool NEED_D = STATS || MAP == RM_CMP_DEPTH, NEED_N = STATS || MAP == RM_CMP_NORMAL || MAP == RM_CMP_SURFACE,
                   NEED_S = STATS || MAP == RM_CMP_SDF, NEED_I = STATS || MAP == RM_CMP_ITERS, IMAGE = MAP != RM_CMP_NONE;
    const unsigned int f = blockIdx.y;
    const long long N = A.npx, first = static_cast<long long>(f) * N;
    const bool has_d = NEED_D && A.depth_a, has_n = NEED_N && A.normal_a, has_s = NEED_S && A.sdf_a, has_i = NEED_I && A.iters_a;
    // the frame's slices (a pair that is absent or not needed: never dereferenced)
    const uint8_t *da = has_d ? A.depth_a + first : nullptr, *db = has_d ? A.depth_b + first : nullptr;
    const uint8_t *na = has_n ? A.normal_a + 3 * first : nullptr, *nb = has_n ? A.normal_b + 3 * first : nullptr;
    const uint16_t *sa = has_s ? A.sdf_a + first : nullptr, *sb = has_s ? A.sdf_b + first : nullptr;
    const uint16_t *ia = has_i ? A.iters_a + first : nullptr, *ib = has_i ? A.iters_b + first : nullptr;
    uint8_t *rgba = IMAGE ? A.rgba + 4 * first : nullptr;
    const bool whole = (reinterpret_cast<uintptr_t>(rgba) & 3) == 0;

    // head: the first pixel of the groups, chosen to 16-byte align as many bytes per pixel as possible
    const uintptr_t addr[9] = {reinterpret_cast<uintptr_t>(da), reinterpret_cast<uintptr_t>(db), reinterpret_cast<uintptr_t>(na),
                               reinterpret_cast<uintptr_t>(nb), reinterpret_cast<uintptr_t>(sa), reinterpret_cast<uintptr_t>(sb),
                               reinterpret_cast<uintptr_t>(ia), reinterpret_cast<uintptr_t>(ib), reinterpret_cast<uintptr_t>(rgba)};
    const bool used[9] = {has_d, has_d, has_n, has_n, has_s, has_s, has_i, has_i, IMAGE};
    constexpr unsigned int bpp[9] = {1, 1, 3, 3, 2, 2, 2, 2, 4};
    unsigned int head = 0, best = 0;
    for (unsigned int h = 0; h < 16; ++h) {
        unsigned int score = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) score += used[k] && ((addr[k] + h * bpp[k]) & 15) == 0 ? bpp[k] : 0u;
        if (score > best) {
            best = score;
            head = h;
        }
    }
    if (head > N) head = static_cast<unsigned int>(N);
    bool vec[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) vec[k] = ((addr[k] + head * bpp[k]) & 15) == 0;
    const long long groups = (N - head) >> 4, tail0 = head + (groups << 4);

    CmpAcc c;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        c.sum[k] = 0;
        c.group[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) c.cnt[k] = 0;
    c.mx[0] = c.mx[1] = 0;

    // head and tail: one pixel per lane of the frame's first workgroup (head + tail < 32)
    if (blockIdx.x == 0) {
        const long long t = threadIdx.x, i = t < head ? t : tail0 + (t - head);
        if (i < N) {
            const unsigned int pna = has_n ? na[3 * i] | na[3 * i + 1] << 8 | na[3 * i + 2] << 16 : 0x808080u;
            const unsigned int pnb = has_n ? nb[3 * i] | nb[3 * i + 1] << 8 | nb[3 * i + 2] << 16 : 0x808080u;
            const unsigned int px = compare_pixel<MAP, STATS>(c, has_d ? da[i] : 0u, has_d ? db[i] : 0u, pna, pnb, has_s ? sa[i] : 0u,
                                                              has_s ? sb[i] : 0u, has_i ? ia[i] : 0u, has_i ? ib[i] : 0u, A.gain);
            if (IMAGE) store_pixel(rgba, i, px, whole);
        }
        if (STATS) fold_group(c);
    }

    const long long step = static_cast<long long>(gridDim.x) * 256;
    for (long long g = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; g < groups; g += step) {
        const long long p0 = head + (g << 4);  // the group's first pixel
        unsigned int wda[4], wdb[4], wna[12], wnb[12], wsa[8], wsb[8], wia[8], wib[8];
        load_group(da + p0, has_d, vec[0], 0u, wda);
        load_group(db + p0, has_d, vec[1], 0u, wdb);
        load_group(na + 3 * p0, has_n, vec[2], 0x80808080u, wna);
        load_group(nb + 3 * p0, has_n, vec[3], 0x80808080u, wnb);
        load_group(sa + p0, has_s, vec[4], 0u, wsa);
        load_group(sb + p0, has_s, vec[5], 0u, wsb);
        load_group(ia + p0, has_i, vec[6], 0u, wia);
        load_group(ib + p0, has_i, vec[7], 0u, wib);
        unsigned int px[16];
#define RM_CMP_PIXEL(P)                                                                                                              \
    px[P] = compare_pixel<MAP, STATS>(c, (wda[(P) >> 2] >> (8 * ((P) & 3))) & 255u, (wdb[(P) >> 2] >> (8 * ((P) & 3))) & 255u,      \
                                      normal_of<P>(wna), normal_of<P>(wnb), (wsa[(P) >> 1] >> (16 * ((P) & 1))) & 0xFFFFu,          \
                                      (wsb[(P) >> 1] >> (16 * ((P) & 1))) & 0xFFFFu, (wia[(P) >> 1] >> (16 * ((P) & 1))) & 0xFFFFu, \
                                      (wib[(P) >> 1] >> (16 * ((P) & 1))) & 0xFFFFu, A.gain);
        RM_CMP_PIXEL(0) RM_CMP_PIXEL(1) RM_CMP_PIXEL(2) RM_CMP_PIXEL(3) RM_CMP_PIXEL(4) RM_CMP_PIXEL(5) RM_CMP_PIXEL(6) RM_CMP_PIXEL(7)
        RM_CMP_PIXEL(8) RM_CMP_PIXEL(9) RM_CMP_PIXEL(10) RM_CMP_PIXEL(11) RM_CMP_PIXEL(12) RM_CMP_PIXEL(13) RM_CMP_PIXEL(14) RM_CMP_PIXEL(15)
#undef RM_CMP_PIXEL
        if (STATS) fold_group(c);
        if (IMAGE) {
            if (vec[8]) {
                uint4 *out = reinterpret_cast<uint4 *>(rgba + 4 * p0);
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = make_uint4(px[4 * k], px[4 * k + 1], px[4 * k + 2], px[4 * k + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) store_pixel(rgba, p0 + k, px[k], whole);
            }
        }
    }

    if (!STATS) return;
    unsigned long long v[CMP_WORDS];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = c.sum[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[5 + k] = c.cnt[k];
    v[W_MAX_DEPTH] = c.mx[0];
    v[W_MAX_NORMAL] = c.mx[1];
    cmp_block_reduce(v);
    if (gridDim.x == 1) {  // the frame's only workgroup
        if (threadIdx.x == 0) cmp_write_record(A.stats + f, N, v);
        return;
    }
    RmComparePartial *partials = A.partials + static_cast<size_t>(f) * gridDim.x;
    unsigned int *counter = A.counters + static_cast<size_t>(f) * gridDim.x;
    __shared__ unsigned int last;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < CMP_WORDS; ++k) __hip_atomic_store(&partials[blockIdx.x].v[k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial record has left before the ticket is taken
        const unsigned int ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = ticket + 1u == gridDim.x;
        if (ticket + 1u == gridDim.x) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... and the invalidate is over before the barrier lets the others load
        }
    }
    __syncthreads();
    if (!last) return;
#pragma unroll
    for (int k = 0; k < CMP_WORDS; ++k) v[k] = 0;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += 256) {
        unsigned long long o[CMP_WORDS];
#pragma unroll
        for (int k = 0; k < CMP_WORDS; ++k) o[k] = __hip_atomic_load(&partials[b].v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cmp_combine(v, o);
    }
    cmp_block_reduce(v);
    if (threadIdx.x == 0) {
        cmp_write_record(A.stats + f, N, v);
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the counter's next user
    }
}

// ------------------------------------------------------------------ hist_kernel (rm_counter_hist_device)
//
// The distribution of the two counters of each frame: 256 bins of min(v >> shift, 255) per counter, with the sum, minimum and
// maximum of the pixels the mask selects and two percentiles derived from the bins.  The shape is compare_kernel's: blockIdx.y
// is the frame, blockIdx.x a share of its pixels, a lane takes GROUPS of 16 consecutive pixels (32 B of each counter, 48 B of
// normal when the mask needs it) with the same head / tail and misaligned-slice handling.
//   * bins: one LDS histogram per WAVE and counter (4 x 2 x 256 words), ds_add without a return value.  The data names the
//     hazard: background pixels all carry one value, so most lanes of most waves of a rendered frame would add 1 at ONE LDS
//     address, and same-address LDS atomics of a wave-instruction serialise.  So nothing is added per pixel: a lane keeps the
//     run in hand (bin, length) per counter in registers, ACROSS its groups, and touches LDS only when the bin changes -- a
//     lane that sees one value makes no LDS access until the end.  At the end the lanes whose run is in the bin of the wave's
//     first lane add their lengths up by __shfl_down and the first lane makes ONE add for them (a constant frame: one add
//     per wave and counter); the others add their own;
//   * sum, min, max: per lane in registers (sums of a group in 32 bits, folded into 64 bits per group), per wave by
//     __shfl_down, per workgroup in LDS, as cmp_block_reduce does;
//   * across workgroups: a frame of one workgroup finishes from its LDS.  Otherwise every lane adds its non-zero bin of each
//     counter to the frame's scratch histogram (RmHistScratch, agent-scope atomics executed at the memory side; sum by add,
//     max and ~min by max, so all-zero is the neutral state), waits for them, and after the barrier the first lane takes a
//     ticket; the workgroup with the last ticket acquires, reads the scratch with all its lanes, leaves it all zero for its
//     next user and finishes.  Integer adds commute: the same bytes whatever the launch shape;
//   * finishing a counter: 256 lanes, one bin each -- an inclusive prefix sum (__shfl_up in the wave, wave totals in LDS), M =
//     the total, r = p (M - 1) / 1000, and the lane with exclusive <= r < inclusive is b_p.  The record is written whole.

struct HistAcc {
    unsigned int bin[2], cnt[2];  // the run in hand
    unsigned int group[2], mn[2], mx[2];
    unsigned long long sum[2];
};

__device__ __forceinline__ void hist_value(HistAcc &a, int c, unsigned int *h, unsigned int v, unsigned int shift) {
    const unsigned int b = min(v >> shift, 255u);
    if (b != a.bin[c]) {  // the run ends: its length goes to the wave's histogram (a first run of length 0 adds 0)
        (void)__hip_atomic_fetch_add(&h[a.bin[c]], a.cnt[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        a.bin[c] = b;
        a.cnt[c] = 0;
    }
    ++a.cnt[c];
    a.group[c] += v;
    a.mn[c] = min(a.mn[c], v);
    a.mx[c] = max(a.mx[c], v);
}

template <bool MASKED>
__device__ __forceinline__ void hist_pixel(HistAcc &a, unsigned int *hs, unsigned int *hi, bool has_s, bool has_i, unsigned int n,
                                           unsigned int s, unsigned int i, unsigned int shift, bool want_surface) {
    if (MASKED && (n != 0x808080u) != want_surface) return;  // raymarcher.ts:97-105
    if (has_s) hist_value(a, 0, hs, s, shift);
    if (has_i) hist_value(a, 1, hi, i, shift);
}

template <bool MASKED>
__global__ __launch_bounds__(256) void hist_kernel(const RmHistArgs A) {
    __shared__ unsigned int bins[4][2][RM_HIST_NBINS];  // [wave][counter][bin]
    __shared__ unsigned long long sh_sum[4][2];
    __shared__ unsigned int sh_mm[4][4], sh_scan[4], sh_pick[2], sh_last;
    const unsigned int f = blockIdx.y, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long long N = A.npx, first = static_cast<long long>(f) * N;
    const bool has_s = A.sdf != nullptr, has_i = A.iters != nullptr, has_n = MASKED, want_surface = A.want_surface != 0;
    const uint16_t *ps = has_s ? A.sdf + first : nullptr, *pi = has_i ? A.iters + first : nullptr;
    const uint8_t *pn = has_n ? A.normal + 3 * first : nullptr;
    for (unsigned int k = t; k < 4 * 2 * RM_HIST_NBINS; k += 256) (&bins[0][0][0])[k] = 0;
    __syncthreads();

    // head: the first pixel of the groups, chosen to 16-byte align as many bytes per pixel as possible (compare_kernel)
    const uintptr_t addr[3] = {reinterpret_cast<uintptr_t>(ps), reinterpret_cast<uintptr_t>(pi), reinterpret_cast<uintptr_t>(pn)};
    const bool used[3] = {has_s, has_i, has_n};
    constexpr unsigned int bpp[3] = {2, 2, 3};
    unsigned int head = 0, best = 0;
    for (unsigned int h = 0; h < 16; ++h) {
        unsigned int score = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) score += used[k] && ((addr[k] + h * bpp[k]) & 15) == 0 ? bpp[k] : 0u;
        if (score > best) {
            best = score;
            head = h;
        }
    }
    if (head > N) head = static_cast<unsigned int>(N);
    bool vec[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vec[k] = ((addr[k] + head * bpp[k]) & 15) == 0;
    const long long groups = (N - head) >> 4, tail0 = head + (groups << 4);

    HistAcc a;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        a.bin[c] = a.cnt[c] = a.group[c] = a.mx[c] = 0;
        a.mn[c] = 0xFFFFFFFFu;
        a.sum[c] = 0;
    }
    unsigned int *hs = bins[wave][0], *hi = bins[wave][1];

    // head and tail: one pixel per lane of the frame's first workgroup (head + tail < 32)
    if (blockIdx.x == 0) {
        const long long i = t < head ? static_cast<long long>(t) : tail0 + (static_cast<long long>(t) - head);
        if (i < N) {
            const unsigned int n = has_n ? pn[3 * i] | pn[3 * i + 1] << 8 | pn[3 * i + 2] << 16 : 0x808080u;
            hist_pixel<MASKED>(a, hs, hi, has_s, has_i, n, has_s ? ps[i] : 0u, has_i ? pi[i] : 0u, A.shift, want_surface);
        }
    }

    const long long step = static_cast<long long>(gridDim.x) * 256;
    for (long long g = static_cast<long long>(blockIdx.x) * 256 + t; g < groups; g += step) {
        const long long p0 = head + (g << 4);  // the group's first pixel
        unsigned int ws[8], wi[8], wn[12];
        load_group(ps + p0, has_s, vec[0], 0u, ws);
        load_group(pi + p0, has_i, vec[1], 0u, wi);
        load_group(pn + 3 * p0, has_n, vec[2], 0x80808080u, wn);
#define RM_HIST_PIXEL(P)                                                                                                          \
    hist_pixel<MASKED>(a, hs, hi, has_s, has_i, normal_of<P>(wn), (ws[(P) >> 1] >> (16 * ((P) & 1))) & 0xFFFFu,                   \
                       (wi[(P) >> 1] >> (16 * ((P) & 1))) & 0xFFFFu, A.shift, want_surface);
        RM_HIST_PIXEL(0) RM_HIST_PIXEL(1) RM_HIST_PIXEL(2) RM_HIST_PIXEL(3) RM_HIST_PIXEL(4) RM_HIST_PIXEL(5) RM_HIST_PIXEL(6) RM_HIST_PIXEL(7)
        RM_HIST_PIXEL(8) RM_HIST_PIXEL(9) RM_HIST_PIXEL(10) RM_HIST_PIXEL(11) RM_HIST_PIXEL(12) RM_HIST_PIXEL(13) RM_HIST_PIXEL(14) RM_HIST_PIXEL(15)
#undef RM_HIST_PIXEL
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            a.sum[c] += a.group[c];
            a.group[c] = 0;
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) a.sum[c] += a.group[c];  // (the head and tail pixels)

    // the runs still in hand: the lanes in the bin of the wave's first lane as ONE add, the others on their own
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const unsigned int lead = __builtin_amdgcn_readfirstlane(a.bin[c]);
        const bool same = a.bin[c] == lead;
        unsigned int merged = same ? a.cnt[c] : 0u;
        for (int off = 32; off > 0; off >>= 1) merged += __shfl_down(merged, off);
        unsigned int *h = bins[wave][c];
        if (lane == 0) (void)__hip_atomic_fetch_add(&h[lead], merged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!same && a.cnt[c]) (void)__hip_atomic_fetch_add(&h[a.bin[c]], a.cnt[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }

    // sums, minima and maxima of the workgroup -> thread 0
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            a.sum[c] += __shfl_down(a.sum[c], off);
            a.mn[c] = min(a.mn[c], static_cast<unsigned int>(__shfl_down(a.mn[c], off)));
            a.mx[c] = max(a.mx[c], static_cast<unsigned int>(__shfl_down(a.mx[c], off)));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            sh_sum[wave][c] = a.sum[c];
            sh_mm[wave][c] = a.mn[c];
            sh_mm[wave][2 + c] = a.mx[c];
        }
    }
    __syncthreads();  // (also: every wave's histogram is complete)
    if (t == 0) {
        for (int w = 1; w < 4; ++w) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                a.sum[c] += sh_sum[w][c];
                a.mn[c] = min(a.mn[c], sh_mm[w][c]);
                a.mx[c] = max(a.mx[c], sh_mm[w][2 + c]);
            }
        }
    }
    unsigned int x[2];  // bin t of each counter
#pragma unroll
    for (int c = 0; c < 2; ++c) x[c] = bins[0][c][t] + bins[1][c][t] + bins[2][c][t] + bins[3][c][t];

    if (gridDim.x > 1) {
        RmHistScratch *S = A.scratch + f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (x[c]) (void)__hip_atomic_fetch_add(&S->bins[c][t], x[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == 0) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                (void)__hip_atomic_fetch_add(&S->sum[c], a.sum[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_max(&S->max[c], a.mx[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_max(&S->inv_min[c], ~a.mn[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this lane's contributions have arrived ...
        __syncthreads();                                  // ... and every lane's, before the ticket is taken
        if (t == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const unsigned int ticket = __hip_atomic_fetch_add(&S->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sh_last = ticket + 1u == gridDim.x;
            if (ticket + 1u == gridDim.x) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // ... and the invalidate is over before the barrier lets the others load
            }
        }
        __syncthreads();
        if (!sh_last) return;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            x[c] = __hip_atomic_load(&S->bins[c][t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&S->bins[c][t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // all zero for the entry's next user
        }
        if (t == 0) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                a.sum[c] = __hip_atomic_load(&S->sum[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a.mx[c] = __hip_atomic_load(&S->max[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a.mn[c] = ~__hip_atomic_load(&S->inv_min[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&S->sum[c], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&S->max[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&S->inv_min[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_store(&S->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // the frame's two records
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        RmCounterHist *rec = c ? &A.hist[f].iters : &A.hist[f].sdf;
        unsigned int incl = x[c];
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned int y = __shfl_up(incl, off);
            if (lane >= static_cast<unsigned int>(off)) incl += y;
        }
        if (lane == 63) sh_scan[wave] = incl;
        if (t == 0) sh_pick[0] = sh_pick[1] = 0;
        __syncthreads();
        unsigned int M = 0;
        for (unsigned int w = 0; w < 4; ++w) {
            if (w < wave) incl += sh_scan[w];
            M += sh_scan[w];
        }
        // b_p: the smallest b with bins[0] + .. + bins[b] > r
        const unsigned long long span = M ? M - 1u : 0u;
        const unsigned int r_lo = static_cast<unsigned int>(A.lo_permille * span / 1000u), r_hi = static_cast<unsigned int>(A.hi_permille * span / 1000u);
        if (M && incl > r_lo && incl - x[c] <= r_lo) sh_pick[0] = t;
        if (M && incl > r_hi && incl - x[c] <= r_hi) sh_pick[1] = t;
        __syncthreads();
        if (t == 0) {
            const unsigned int mn = M ? a.mn[c] : 0u, mx = M ? a.mx[c] : 0u, b_lo = sh_pick[0], b_hi = sh_pick[1];
            rec->pixels = M;
            rec->sum = M ? a.sum[c] : 0ull;
            rec->min = mn;
            rec->max = mx;
            rec->range_lo = M ? max(mn, b_lo << A.shift) : 0u;
            rec->range_hi = !M ? 0u : b_hi == 255u ? mx : min(mx, ((b_hi + 1u) << A.shift) - 1u);
            rec->shift = A.shift;
            rec->reserved = 0;
        }
        rec->bins[t] = x[c];
        __syncthreads();  // (sh_scan and sh_pick are written again for the second counter)
    }
}

// ------------------------------------------------------------------ shade_ranged_kernel (rm_shade_ranged_device)
//
// The heatmap ramp of IterationHeatmap.ts:26-29 over a range instead of counter * 5 % 256: s = 0 up to lo, 255 from hi,
// (v - lo) * 255 / (hi - lo) between.  One pass, 2 B read and 4 B written per pixel: a lane takes groups of 8 pixels (one 16-byte
// load, two 16-byte stores) that start `head` pixels into the frame, where the counter slice is 16-byte aligned; an image slice
// that is misaligned there is stored pixel by pixel; head and tail (< 16 pixels) go to the first lanes of the frame's first
// workgroup.  lo and hi are the same for the whole workgroup: the kernel arguments, or two scalar loads from the frame's
// record.  The division is by a workgroup-uniform d = hi - lo and of n = (v - lo) * 255 < 2^24: with d <= 2^L, k = 24 + L and
// m = ceil(2^k / d) < 2^25 + 1, (n * m) >> k == n / d exactly (m d - 2^k < d <= 2^L, so n (m d - 2^k) < 2^k).
__device__ __forceinline__ unsigned int ranged_pixel(unsigned int v, unsigned int lo, unsigned int hi, unsigned int m, unsigned int k) {
    const unsigned int q = static_cast<unsigned int>((static_cast<unsigned long long>((v - lo) * 255u) * m) >> k);
    const unsigned int s = v <= lo ? 0u : v >= hi ? 255u : q;
    return 0xFF000000u | min(2u * s, 255u) | (min(512u - 2u * s, 255u) << 8);
}

__global__ __launch_bounds__(256) void shade_ranged_kernel(const RmShadeRangedArgs A) {
    const unsigned int f = blockIdx.y, t = threadIdx.x;
    const long long N = A.npx, first = static_cast<long long>(f) * N;
    const uint16_t *val = A.values + first;
    uint8_t *rgba = A.rgba + 4 * first;
    unsigned int lo = A.lo, hi = A.hi;
    if (A.hist) {
        const RmCounterHist *rec = A.counter ? &A.hist[f].iters : &A.hist[f].sdf;
        lo = rec->range_lo;
        hi = rec->range_hi;
    }
    const unsigned int d = hi > lo ? hi - lo : 1u;
    const unsigned int k = 24u + (d > 1u ? 32u - static_cast<unsigned int>(__builtin_clz(d - 1u)) : 0u);
    const unsigned long long pow2 = 1ull << k;
    unsigned int m = static_cast<unsigned int>(static_cast<double>(pow2) / static_cast<double>(d));  // ceil(2^k / d), made exact below
    while (static_cast<unsigned long long>(m) * d < pow2) ++m;
    while (m > 1u && static_cast<unsigned long long>(m - 1u) * d >= pow2) --m;

    const bool whole = (reinterpret_cast<uintptr_t>(rgba) & 3) == 0;
    unsigned int head = static_cast<unsigned int>(((16u - (reinterpret_cast<uintptr_t>(val) & 15u)) & 15u) >> 1);
    if (head > N) head = static_cast<unsigned int>(N);
    const bool vec_in = ((reinterpret_cast<uintptr_t>(val) + 2 * head) & 15) == 0, vec_out = ((reinterpret_cast<uintptr_t>(rgba) + 4 * head) & 15) == 0;
    const long long groups = (N - head) >> 3, tail0 = head + (groups << 3);
    if (blockIdx.x == 0) {
        const long long i = t < head ? static_cast<long long>(t) : tail0 + (static_cast<long long>(t) - head);
        if (i < N) store_pixel(rgba, i, ranged_pixel(val[i], lo, hi, m, k), whole);
    }
    const long long step = static_cast<long long>(gridDim.x) * 256;
    for (long long g = static_cast<long long>(blockIdx.x) * 256 + t; g < groups; g += step) {
        const long long p0 = head + (g << 3);
        unsigned int w[4], px[8];
        load_group(val + p0, true, vec_in, 0u, w);
#pragma unroll
        for (int p = 0; p < 8; ++p) px[p] = ranged_pixel((w[p >> 1] >> (16 * (p & 1))) & 0xFFFFu, lo, hi, m, k);
        if (vec_out) {
            uint4 *out = reinterpret_cast<uint4 *>(rgba + 4 * p0);
            out[0] = make_uint4(px[0], px[1], px[2], px[3]);
            out[1] = make_uint4(px[4], px[5], px[6], px[7]);
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) store_pixel(rgba, p0 + p, px[p], whole);
        }
    }
}

// ------------------------------------------------------------------ shade_lit_kernel (rm_shade_lit_device)
//
// PhongModel.shade (rm_device.h, shade_phong_lit) with the light and occlusion terms of a light query: blockIdx.y is the frame,
// the frame's workgroups stride over its pixels, one pixel per lane and trip.  Not HBM-bound like its neighbours (12 B read,
// 4 B written against two square roots and a binary64 pow per pixel), so the pixels are not grouped for wide loads.
__global__ __launch_bounds__(256) void shade_lit_kernel(const RmShadeLitArgs A) {
    const long long N = A.npx, first = static_cast<long long>(blockIdx.y) * N;
    const uint8_t *depth = A.depth + first, *normal = A.normal + 3 * first;
    const float *lit = A.lit + first, *ao = A.ao + first;
    uint8_t *rgba = A.rgba + 4 * first;
    const bool whole = (reinterpret_cast<uintptr_t>(rgba) & 3) == 0;
    const long long step = static_cast<long long>(gridDim.x) * 256;
    for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < N; i += step) {
        const uchar4 c = rmd::shade_phong_lit(depth[i], normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], A.light[0], A.light[1], A.light[2],
                                              static_cast<double>(lit[i]), static_cast<double>(ao[i]));
        store_pixel(rgba, i, c.x | (static_cast<unsigned int>(c.y) << 8) | (static_cast<unsigned int>(c.z) << 16) | (static_cast<unsigned int>(c.w) << 24), whole);
    }
}

// ------------------------------------------------------------------ shade_field_kernel (rm_shade_field_device)
//
// The slice image of a field query: one value in (a binary64 distance or a u32 evaluation count), one pixel out, the
// workgroups stride over the n values.  DISTANCE: two binary64 quotients (|d| / range, |d| / band), everything after them in
// integers -- intensity 96 .. 255 by |d|, every second iso-band a quarter darker, blue inside and orange outside, a white zero
// line, magenta for NaN.  COUNT: shade_ranged_kernel's s and ramp over (lo, hi), the quotient taken in 64 bits.
__device__ __forceinline__ unsigned int field_distance_pixel(double d, double range, double band, double line) {
    if (d != d) return 0xFFFF00FFu;
    const double a = __builtin_fabs(d);
    if (a < line) return 0xFFFFFFFFu;
    const double x = a / range, y = a / band;
    const int s = x >= 1.0 ? 255 : static_cast<int>(x * 255.0);
    int I = 96 + 159 * s / 255;
    const int q = y < 2147483648.0 ? static_cast<int>(y) : 0;
    if (q & 1) I = I * 3 / 4;
    const bool inside = d < 0.0;  // -0.0 counts as outside
    const unsigned int r = (inside ? 60 : 230) * I / 255, g = (inside ? 120 : 140) * I / 255, b = (inside ? 230 : 50) * I / 255;
    return 0xFF000000u | r | (g << 8) | (b << 16);
}

__device__ __forceinline__ unsigned int field_count_pixel(unsigned int v, unsigned int lo, unsigned int hi) {
    const unsigned int s = v <= lo ? 0u : v >= hi ? 255u : static_cast<unsigned int>(static_cast<unsigned long long>(v - lo) * 255ull / (hi - lo));
    return 0xFF000000u | min(2u * s, 255u) | (min(512u - 2u * s, 255u) << 8);
}

__global__ __launch_bounds__(256) void shade_field_kernel(const RmShadeFieldArgs A) {
    const bool whole = (reinterpret_cast<uintptr_t>(A.rgba) & 3) == 0;
    const long long step = static_cast<long long>(gridDim.x) * 256;
    for (long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; i < A.n; i += step) {
        const unsigned int px = A.map == 0 ? field_distance_pixel(static_cast<const double *>(A.values)[i], A.range, A.band, A.line)
                                           : field_count_pixel(static_cast<const unsigned int *>(A.values)[i], A.lo, A.hi);
        store_pixel(A.rgba, i, px, whole);
    }
}

}  // namespace

hipError_t rm_launch_assemble(const unsigned char *gathered, int64_t rank_stride, int64_t section_offset, int32_t row_bytes,
                              int32_t height, int32_t stripe_rows, const int32_t *stripe_src, int32_t n_stripes,
                              unsigned char *frame, int64_t acc_offset, int32_t world, RmDiagDevice *acc, hipStream_t stream) {
    if (n_stripes <= 0 && !(acc && acc_offset >= 0)) return hipSuccess;
    // ~1024 workgroups (4 per CU) whatever the stripe height
    int chunks = n_stripes > 0 ? (1024 + n_stripes - 1) / n_stripes : 1;
    const long long stripe_bytes = static_cast<long long>(stripe_rows) * row_bytes;
    const long long max_chunks = (stripe_bytes / 16 + 255) / 256;
    if (chunks > max_chunks) chunks = static_cast<int>(max_chunks > 0 ? max_chunks : 1);
    const unsigned blocks = static_cast<unsigned>((n_stripes > 0 ? n_stripes : 1) * chunks);
    hipLaunchKernelGGL(assemble_kernel, dim3(blocks), dim3(256), 0, stream, gathered, static_cast<long long>(rank_stride),
                       static_cast<long long>(section_offset), row_bytes, height, stripe_rows, stripe_src, n_stripes, frame,
                       static_cast<long long>(acc_offset), world, acc, chunks);
    return hipGetLastError();
}


int32_t rm_compare_blocks_per_frame(int64_t npx, int32_t n_frames) {
    // ~2048 workgroups per launch, at most 512 per frame (two per CU: all resident at the kernel's three waves per SIMD, and
    // the frame's last workgroup adds up that many partial records), never more than the frame has groups for
    const int64_t want = (npx / 16 + 255) / 256, share = n_frames > 0 ? 2048 / n_frames : 1;
    const int64_t cap = share > 512 ? 512 : share;
    return static_cast<int32_t>(want < 1 || cap < 1 ? 1 : want < cap ? want : cap);
}

hipError_t rm_launch_compare(const RmCompareArgs &a, int32_t map, int32_t n_frames, int32_t blocks_per_frame, hipStream_t stream,
                             const char **kernel_name) {
    const bool stats = a.stats != nullptr;
    if (n_frames <= 0 || a.npx <= 0 || (map == RM_CMP_NONE && !stats)) return hipSuccess;
    const dim3 grid(static_cast<unsigned>(blocks_per_frame), static_cast<unsigned>(n_frames)), block(256);
    const char *name = nullptr;
#define RM_CMP_CASE(M)                                                                                \
    case M:                                                                                           \
        if (stats) {                                                                                  \
            hipLaunchKernelGGL((compare_kernel<M, true>), grid, block, 0, stream, a);                 \
            name = "compare_kernel<" #M ", true>";                                                    \
        } else {                                                                                      \
            hipLaunchKernelGGL((compare_kernel<M, false>), grid, block, 0, stream, a);                \
            name = "compare_kernel<" #M ", false>";                                                   \
        }                                                                                             \
        break;
    switch (map) {
        RM_CMP_CASE(0) RM_CMP_CASE(1) RM_CMP_CASE(2) RM_CMP_CASE(3) RM_CMP_CASE(4)
    case RM_CMP_NONE:
        hipLaunchKernelGGL((compare_kernel<RM_CMP_NONE, true>), grid, block, 0, stream, a);
        name = "compare_kernel<-1, true>";
        break;
    default: return hipErrorInvalidValue;
    }
#undef RM_CMP_CASE
    if (kernel_name) *kernel_name = name;
    return hipGetLastError();
}


hipError_t rm_launch_hist(const RmHistArgs &a, bool masked, int32_t n_frames, int32_t blocks_per_frame, hipStream_t stream,
                          const char **kernel_name) {
    if (n_frames <= 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>(blocks_per_frame), static_cast<unsigned>(n_frames)), block(256);
    if (masked) hipLaunchKernelGGL((hist_kernel<true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((hist_kernel<false>), grid, block, 0, stream, a);
    if (kernel_name) *kernel_name = masked ? "hist_kernel<true>" : "hist_kernel<false>";
    return hipGetLastError();
}

int32_t rm_shade_ranged_blocks_per_frame(int64_t npx, int32_t n_frames) {
    // ~4096 workgroups per launch, at most 2048 per frame (a lane of a 4K frame takes two groups), never more than the frame has groups for
    const int64_t want = (npx / 8 + 255) / 256, share = n_frames > 0 ? 4096 / n_frames : 1;
    const int64_t cap = share > 2048 ? 2048 : share;
    return static_cast<int32_t>(want < 1 || cap < 1 ? 1 : want < cap ? want : cap);
}

hipError_t rm_launch_shade_ranged(const RmShadeRangedArgs &a, int32_t n_frames, hipStream_t stream, const char **kernel_name) {
    if (n_frames <= 0 || a.npx <= 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>(rm_shade_ranged_blocks_per_frame(a.npx, n_frames)), static_cast<unsigned>(n_frames)), block(256);
    hipLaunchKernelGGL(shade_ranged_kernel, grid, block, 0, stream, a);
    if (kernel_name) *kernel_name = "shade_ranged_kernel";
    return hipGetLastError();
}

hipError_t rm_launch_shade_lit(const RmShadeLitArgs &a, int32_t n_frames, hipStream_t stream, const char **kernel_name) {
    if (n_frames <= 0 || a.npx <= 0) return hipSuccess;
    // ~4096 workgroups per launch, never more than a frame has pixels for
    const int64_t want = (a.npx + 255) / 256, share = 4096 / n_frames;
    const int64_t per_frame = want < share ? want : (share < 1 ? 1 : share);
    const dim3 grid(static_cast<unsigned>(per_frame), static_cast<unsigned>(n_frames)), block(256);
    hipLaunchKernelGGL(shade_lit_kernel, grid, block, 0, stream, a);
    if (kernel_name) *kernel_name = "shade_lit_kernel";
    return hipGetLastError();
}

hipError_t rm_launch_shade_field(const RmShadeFieldArgs &a, hipStream_t stream, const char **kernel_name) {
    if (a.n <= 0) return hipSuccess;
    // ~4096 workgroups per launch, never more than there are values for
    const int64_t want = (a.n + 255) / 256;
    const dim3 grid(static_cast<unsigned>(want < 4096 ? want : 4096)), block(256);
    hipLaunchKernelGGL(shade_field_kernel, grid, block, 0, stream, a);
    if (kernel_name) *kernel_name = "shade_field_kernel";
    return hipGetLastError();
}
