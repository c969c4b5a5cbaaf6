// rm_parts.hip -- the connected parts of a solid on a lattice (gfx950): rm_label_field_device labels the 6-connected components of
// the points on one side of iso, rm_measure_labels_device gives every part an rm_measure of its own.
//
// The rule is the contract of include/rm_raymarch.h ("parts"); tests/parts_model.py restates it in numpy.  Labels, counts and
// sums are integers with one right answer, so nothing here depends on the order in which atomics arrive.  Work is mapped by
// lattice point as in rm_mesh.hip: a workgroup covers 256 consecutive linear indices, a wave 64 of them.  d_labels itself is the
// union-find's parent array; a parent is the linear index of a point of the same part, never above the point's own.
//   parts_init_kernel<T>    membership by ballot; every point of the set points at the start of its run within the wave and row
//   parts_merge_kernel      unions with the -j and -k neighbours, and with -i where a run was cut at a wave's lane 0
//   parts_flatten_kernel    parent[l] = root(l); roots and points of the set per workgroup
//   parts_scan_kernel       one workgroup: exclusive scan of the root totals (in place); n_points, n_set, n_parts into the info
//   parts_number_kernel     a root's number: its workgroup's offset plus its ballot rank, into the map
//   parts_relabel_kernel    labels[l] = map[labels[l]]
//   parts_records_kernel    the empty record, n_records times
//   parts_measure_kernel    a persistent grid of waves over contiguous spans of 64-point chunks: the sums of every part
// No wave waits for another: the only loops that depend on other threads are find and unite below; every step of either lowers
// an index, and each thread has a budget of n hops after which it raises info.gave_up and stops (DESIGN.md 4 has the argument).
// parent[] is read through relaxed agent-scope atomic loads inside those loops and written by atomicMin and relaxed atomic stores
// alone; kernel boundaries separate the phases.
#include <hip/hip_runtime.h>

#include <climits>

#include "rm_mesh_device.h"

namespace {

__device__ __forceinline__ int load_parent(const int *at) { return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void give_up(RmPartsInfo *info) { atomicOr(reinterpret_cast<unsigned long long *>(&info->gave_up), 1ull); }

// x -> the root of x's tree as this thread sees it (a parent is below its child, so x only falls); false: the budget ran out
__device__ __forceinline__ bool find_root(const int *parent, int &x, unsigned &budget) {
    for (;;) {
        const int p = load_parent(parent + x);
        if (p >= x) return true;  // p == x: a root (p > x never happens)
        x = p;
        if (--budget == 0u) return false;
    }
}

// Joins the trees of a and b.  The larger root is linked below the smaller by atomicMin, whose returned value says whether it
// still was a root; if it was not, what it pointed at and the smaller root remain to be joined, and both lie below it: the larger
// index of the pair falls with every round.  The root of a finished tree is therefore its smallest index, whatever the order.
__device__ __forceinline__ void unite(int *parent, int a, int b, unsigned &budget, RmPartsInfo *info) {
    for (;;) {
        if (!find_root(parent, a, budget) || !find_root(parent, b, budget)) break;
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
        if (--budget == 0u) break;
    }
    give_up(info);
}

struct Point {
    unsigned i, j, k;
};
__device__ __forceinline__ Point locate(unsigned l, unsigned nu, unsigned nv) {
    Point p;
    const unsigned row = l / nu;
    p.i = l - row * nu;
    p.k = row / nv;
    p.j = row - p.k * nv;
    return p;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void parts_init_kernel(RmPartsArgs a) {
    const unsigned l = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = l < a.n;
    bool in = false;
    if (valid) {
        const double v = static_cast<double>(static_cast<const T *>(a.values)[l]);  // binary32 widens exactly
        in = a.outside ? !(v < a.iso) : v < a.iso;
    }
    const unsigned long long set = __ballot(in), row_start = __ballot(valid && l % a.nu == 0u);
    // a run starts where the set does, and at a row's first point: bit p of `starts`
    const unsigned long long starts = set & ~((set << 1) & ~row_start);
    if (!valid) return;
    int parent = -1;
    if (in) {
        const unsigned long long below = starts & ((2ull << lane) - 1ull);  // lane 63: 2 << 63 is 0, all bits
        parent = static_cast<int>(l - lane + (63u - static_cast<unsigned>(__clzll(static_cast<long long>(below)))));
    }
    a.labels[l] = parent;
}

__global__ __launch_bounds__(kBlock) void parts_merge_kernel(RmPartsArgs a) {
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= a.n) return;
    int *parent = a.labels;
    // whether a point is in the set is the sign of its word, which the init kernel fixed: plain loads
    if (parent[l] < 0) return;
    const Point p = locate(l, a.nu, a.nv);
    const unsigned plane = a.nu * a.nv;
    unsigned budget = static_cast<unsigned>(a.n);
    const bool left = p.i > 0u && parent[l - 1u] >= 0;
    // l - 1 is in l's run unless the wave began between them
    if (left && (threadIdx.x & 63u) == 0u) unite(parent, static_cast<int>(l), static_cast<int>(l - 1u), budget, a.info);
    // with l - 1 and its lower neighbour both in the set, l ~ l - 1 ~ its lower neighbour ~ l's lower neighbour already
    if (p.j > 0u && parent[l - a.nu] >= 0 && !(left && parent[l - 1u - a.nu] >= 0))
        unite(parent, static_cast<int>(l), static_cast<int>(l - a.nu), budget, a.info);
    if (p.k > 0u && parent[l - plane] >= 0 && !(left && parent[l - 1u - plane] >= 0))
        unite(parent, static_cast<int>(l), static_cast<int>(l - plane), budget, a.info);
}

__global__ __launch_bounds__(kBlock) void parts_flatten_kernel(RmPartsArgs a) {
    __shared__ unsigned s_sums[2][kWaves];
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    int root = l < a.n ? load_parent(a.labels + l) : -1;
    const bool in[1] = {root >= 0};
    if (in[0]) {
        unsigned budget = static_cast<unsigned>(a.n);
        root = static_cast<int>(l);
        if (!find_root(a.labels, root, budget)) give_up(a.info);
        // whoever walks through l meanwhile reads the old parent or the root: both are in l's part and not above l
        __hip_atomic_store(a.labels + l, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool is_root[1] = {in[0] && root == static_cast<int>(l)};
    unsigned n_roots, n_set;
    block_rank<1>(is_root, s_sums[0], &n_roots);
    block_rank<1>(in, s_sums[1], &n_set);
    if (threadIdx.x == 0) {
        a.totals[blockIdx.x] = n_roots;
        a.totals[a.n_blocks + blockIdx.x] = n_set;
    }
}

__global__ __launch_bounds__(kScan) void parts_scan_kernel(uint32_t *totals, unsigned n_blocks, RmPartsInfo *info, long long n) {
    __shared__ unsigned s_sums[2][kScan / 64];
    unsigned long long roots = 0, set = 0;
    for (unsigned base = 0; base < n_blocks; base += kScan) {
        const unsigned at = base + threadIdx.x;
        const unsigned r = at < n_blocks ? totals[at] : 0u, s = at < n_blocks ? totals[n_blocks + at] : 0u;
        unsigned sum_r, sum_s;
        const unsigned inclusive = scan_step(r, s_sums[0], &sum_r);
        scan_step(s, s_sums[1], &sum_s);
        if (at < n_blocks) totals[at] = static_cast<uint32_t>(roots + (inclusive - r));  // at most 2^30 roots
        roots += sum_r;
        set += sum_s;
        __syncthreads();  // the next step writes s_sums again
    }
    if (threadIdx.x == 0) {  // gave_up stays what the kernels ahead made of the zero it started from
        info->n_points = n;
        info->n_set = static_cast<long long>(set);
        info->n_parts = static_cast<long long>(roots);
    }
}

__global__ __launch_bounds__(kBlock) void parts_number_kernel(RmPartsArgs a) {
    __shared__ unsigned s_sums[kWaves];
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    const bool is_root[1] = {l < a.n && a.labels[l] == static_cast<int>(l)};
    unsigned total;
    const unsigned r = a.totals[blockIdx.x] + block_rank<1>(is_root, s_sums, &total);
    if (is_root[0]) a.map[l] = r;
}

__global__ __launch_bounds__(kBlock) void parts_relabel_kernel(RmPartsArgs a) {
    const unsigned l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= a.n) return;
    const int root = a.labels[l];  // below n whatever happened: every parent is a lattice index
    if (root >= 0) a.labels[l] = static_cast<int>(a.map[root]);
}

// ---- a record per part

// the sums of a record in the order they are carried: n_inside, sum1, sum2, crossings
enum { P_INSIDE, P_I, P_J, P_K, P_II, P_JJ, P_KK, P_IJ, P_JK, P_KI, P_CROSS_I, P_CROSS_J, P_CROSS_K, P_COUNT };

struct IndexBox {
    int lo[3], hi[3];
    __device__ void clear() {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = INT_MAX;
            hi[c] = -1;
        }
    }
};

__global__ __launch_bounds__(kBlock) void parts_records_kernel(RmPartsMeasureArgs a) {
    const unsigned r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= a.n_records) return;
    RmMeasure m = {};
    m.n_points = a.n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m.lo[c] = INT_MAX;
        m.hi[c] = -1;
    }
    a.records[r] = m;
}

// Integer atomics: the record does not depend on who arrives first.  A sum of zero and a box that cannot move are not sent.
__device__ __forceinline__ void add_to_record(RmMeasure *rec, const long long (&sum)[P_COUNT], const IndexBox &box) {
    long long *field = &rec->n_inside;
#pragma unroll
    for (int n = 0; n < P_COUNT; ++n) {
        // n_inside, (n_nonfinite), sum1, sum2, crossings follow one another in the record
        long long *at = field + (n == 0 ? 0 : n + 1);
        if (sum[n]) atomicAdd(reinterpret_cast<unsigned long long *>(at), static_cast<unsigned long long>(sum[n]));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        atomicMin(&rec->lo[c], box.lo[c]);
        atomicMax(&rec->hi[c], box.hi[c]);
    }
}

// the wave's lanes -> lane 0, which adds them to the record of part `label`
__device__ __forceinline__ void flush(const RmPartsMeasureArgs &a, int label, long long (&sum)[P_COUNT], IndexBox &box) {
#pragma unroll
    for (unsigned d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int n = 0; n < P_COUNT; ++n) sum[n] += __shfl_down(sum[n], d);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            box.lo[c] = min(box.lo[c], __shfl_down(box.lo[c], d));
            box.hi[c] = max(box.hi[c], __shfl_down(box.hi[c], d));
        }
    }
    if ((threadIdx.x & 63u) == 0u) add_to_record(a.records + label, sum, box);
#pragma unroll
    for (int n = 0; n < P_COUNT; ++n) sum[n] = 0;
    box.clear();
}

// the product of two 32-bit factors in 64 bits
__device__ __forceinline__ long long wide(unsigned x, unsigned y) { return static_cast<long long>(static_cast<unsigned long long>(x) * y); }

// A wave takes the chunks first .. first + per_wave - 1 of 64 consecutive points.  Where all the points of a chunk that have a
// record carry one label -- a solid in few pieces: nearly everywhere -- every lane adds its own point to sums it keeps in
// registers, and the wave sends them once, when the label changes or its span ends.  Else the first lane of every run of one
// label within a row sends the run's closed forms, its crossings counted from ballots.
__global__ __launch_bounds__(kBlock) void parts_measure_kernel(RmPartsMeasureArgs a, unsigned chunks, unsigned per_wave) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = blockIdx.x * kWaves + static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    const unsigned long long first_chunk = static_cast<unsigned long long>(wave) * per_wave;
    const unsigned first = static_cast<unsigned>(first_chunk < chunks ? first_chunk : chunks), last = min(first + per_wave, chunks);
    const unsigned plane = a.nu * a.nv;
    const int32_t *labels = a.labels;
    long long sum[P_COUNT];
#pragma unroll
    for (int n = 0; n < P_COUNT; ++n) sum[n] = 0;
    IndexBox box;
    box.clear();
    int current = -1;  // the label the sums belong to (wave-uniform)
    for (unsigned chunk = first; chunk < last; ++chunk) {
        const unsigned l = chunk * 64u + lane;
        const int label = l < a.n ? labels[l] : -1;
        const bool in = label >= 0, use = in && static_cast<unsigned>(label) < a.n_records;
        const unsigned long long used = __ballot(use);
        if (used == 0ull) continue;
        const Point p = locate(l, a.nu, a.nv);
        // the lattice edges at the point whose other end is not in the set, towards -A and towards +A
        bool out_lo[3], out_hi[3];
        out_lo[0] = in && p.i > 0u && labels[l - 1u] < 0;
        out_hi[0] = in && p.i + 1u < a.nu && labels[l + 1u] < 0;
        out_lo[1] = in && p.j > 0u && labels[l - a.nu] < 0;
        out_hi[1] = in && p.j + 1u < a.nv && labels[l + a.nu] < 0;
        out_lo[2] = in && p.k > 0u && labels[l - plane] < 0;
        out_hi[2] = in && p.k + 1u < a.nw && labels[l + plane] < 0;
        const int one = __shfl(label, __ffsll(static_cast<long long>(used)) - 1);
        if (__ballot(use && label != one) == 0ull) {
            if (one != current) {
                if (current >= 0) flush(a, current, sum, box);
                current = one;
            }
            if (use) {  // i, j, k < 2^16: every product fits 32 bits
                sum[P_INSIDE] += 1;
                sum[P_I] += p.i;
                sum[P_J] += p.j;
                sum[P_K] += p.k;
                sum[P_II] += p.i * p.i;
                sum[P_JJ] += p.j * p.j;
                sum[P_KK] += p.k * p.k;
                sum[P_IJ] += p.i * p.j;
                sum[P_JK] += p.j * p.k;
                sum[P_KI] += p.k * p.i;
                const unsigned at[3] = {p.i, p.j, p.k};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sum[P_CROSS_I + c] += (out_lo[c] ? 1 : 0) + (out_hi[c] ? 1 : 0);
                    box.lo[c] = min(box.lo[c], static_cast<int>(at[c]));
                    box.hi[c] = max(box.hi[c], static_cast<int>(at[c]));
                }
            }
            continue;
        }
        // several labels: a run is a maximal span of lanes with one label within a row
        const int before = __shfl_up(label, 1);
        const bool head = use && (lane == 0u || p.i == 0u || before != label);
        const unsigned long long ends = __ballot(head || !use);
        unsigned long long cross_lo[3], cross_hi[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cross_lo[c] = __ballot(out_lo[c]);
            cross_hi[c] = __ballot(out_hi[c]);
        }
        if (!head) continue;
        const unsigned long long above = ends & ~((2ull << lane) - 1ull);  // lane 63: none
        const unsigned count = (above ? static_cast<unsigned>(__ffsll(static_cast<long long>(above))) - 1u : 64u) - lane;
        const unsigned long long run = (count == 64u ? ~0ull : (1ull << count) - 1ull) << lane;
        // the sums of i and of i * i over i = p.i .. p.i + count - 1; count <= 64 and i < 2^16
        const unsigned tri = count * (count - 1u) / 2u, sum_i = count * p.i + tri;
        const unsigned long long sum_ii = static_cast<unsigned long long>(count) * p.i * p.i + static_cast<unsigned long long>(p.i) * (2u * tri) +
                                          (count - 1u) * count * (2u * count - 1u) / 6u;
        long long run_sum[P_COUNT];
        run_sum[P_INSIDE] = count;
        run_sum[P_I] = sum_i;
        run_sum[P_J] = p.j * count;
        run_sum[P_K] = p.k * count;
        run_sum[P_II] = static_cast<long long>(sum_ii);
        run_sum[P_JJ] = wide(p.j * p.j, count);
        run_sum[P_KK] = wide(p.k * p.k, count);
        run_sum[P_IJ] = wide(p.j, sum_i);
        run_sum[P_JK] = wide(p.j * count, p.k);
        run_sum[P_KI] = wide(p.k, sum_i);
#pragma unroll
        for (int c = 0; c < 3; ++c) run_sum[P_CROSS_I + c] = __popcll(cross_lo[c] & run) +__popcll(cross_hi[c] & run);
        IndexBox run_box;
        run_box.lo[0] = static_cast<int>(p.i);
        run_box.hi[0] = static_cast<int>(p.i + count - 1u);
        run_box.lo[1] = run_box.hi[1] = static_cast<int>(p.j);
        run_box.lo[2] = run_box.hi[2] = static_cast<int>(p.k);
        add_to_record(a.records + label, run_sum, run_box);
    }
    if (current >= 0) flush(a, current, sum, box);
}

template <typename T>
hipError_t launch_label(const RmPartsArgs &a, hipStream_t stream) {
    const dim3 grid(a.n_blocks), block(kBlock);
    hipLaunchKernelGGL(parts_init_kernel<T>, grid, block, 0, stream, a);
    hipLaunchKernelGGL(parts_merge_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(parts_flatten_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(parts_scan_kernel, dim3(1), dim3(kScan), 0, stream, a.totals, a.n_blocks, a.info, a.n);
    hipLaunchKernelGGL(parts_number_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(parts_relabel_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t rm_launch_label_field(const RmPartsArgs &a, hipStream_t stream, const char **kernel_name) {
    if (a.n <= 0 || a.n > (1ll << 30) || a.n_blocks != static_cast<unsigned>((a.n + kBlock - 1) / kBlock)) return hipErrorInvalidValue;
    if (kernel_name) *kernel_name = "parts_relabel_kernel";
    return a.f32 ? launch_label<float>(a, stream) : launch_label<double>(a, stream);
}

hipError_t rm_launch_measure_labels(const RmPartsMeasureArgs &a, int num_cus, hipStream_t stream, const char **kernel_name) {
    if (a.n < 0 || a.n > (1ll << 30) || a.n_records > RM_PARTS_MAX_RECORDS) return hipErrorInvalidValue;
    if (a.n_records == 0) return hipSuccess;
    if (kernel_name) *kernel_name = a.n > 0 ? "parts_measure_kernel" : "parts_records_kernel";
    hipLaunchKernelGGL(parts_records_kernel, dim3((a.n_records + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
    if (a.n > 0) {
        // four workgroups a CU at most: a wave that keeps one label sends its sums once, so fewer waves send fewer atomics
        const unsigned chunks = static_cast<unsigned>((a.n + 63) / 64), most = 4u * kWaves * static_cast<unsigned>(num_cus > 0 ? num_cus : 256);
        const unsigned per_wave = (chunks + most - 1u) / most, waves = (chunks + per_wave - 1u) / per_wave;
        hipLaunchKernelGGL(parts_measure_kernel, dim3((waves + kWaves - 1u) / kWaves), dim3(kBlock), 0, stream, a, chunks, per_wave);
    }
    return hipGetLastError();
}
