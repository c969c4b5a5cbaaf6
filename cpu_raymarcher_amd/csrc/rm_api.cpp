// rm_api.cpp -- the C ABI of include/rm_raymarch.h on top of the HIP kernels.
//
// Host side of the tile dispatch (reference src/workers/raymarchWorker.ts:33-92): a job
// names (preset, accel, camera angles, row range); the ctx keeps the built scene resident
// in HBM and rebuilds it only when (preset, accel) changes -- the reference rebuilds it
// twice per tile per frame (scene.ts:24-29 then raymarchWorker.ts:38).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <unordered_map>
#include <new>
#include <string>
#include <vector>

#include "../../include/rm_raymarch.h"
#include "rm_diag.h"
#include "rm_kernels.h"
#include "rm_rtc.h"
#include "rm_scene_host.h"

namespace {

// Every table of the device-resident scene, once: X(name, always) -- HostScene::name is uploaded to DeviceScene::name, a pointer
// to the same element type.  `always` 0: an empty table stays a null pointer (slot_object: null says that device slots are
// object indices).
#define RM_SCENE_ARRAYS(X)                                                                                                        \
    X(spheres, 1) X(radii, 1) X(bvh, 1) X(bvh_prims, 1) X(oct, 1) X(oct_prims, 1) X(pq_cells, 1) X(pq_list, 1) X(nn_cells, 1)      \
    X(nn_list, 1) X(prims, 1) X(prog, 1) X(obj_ranges, 1) X(oct_recs, 1) X(oct_lut, 1) X(oct_sub_hdr, 1) X(oct_sub_list, 1)       \
    X(slot_object, 0) X(ext_cells, 1) X(ext_list, 1) X(step_tab, 1) X(cell_tab, 1)

struct DeviceScene {
#define RM_X(name, always) decltype(rmh::HostScene::name)::value_type *name = nullptr;
    RM_SCENE_ARRAYS(RM_X)
#undef RM_X
    uint16_t *bvh_leaves = nullptr;  // node indices of the non-empty BVH leaves, increasing (v2 bundle cull: cull_leaf_table)
    int32_t bvh_leaf_count = 0;      // 0: no cull (no BVH, too many leaves, or a leaf box not inside its ancestors')
};

// What a scene is built from, in one of the three shapes the builders of rm_scene_host.h take: an upload as it was given, or
// a preset's objects.
struct SceneDesc {
    enum Kind { kSpheres, kPrims, kNodes } kind = kSpheres;
    std::vector<float> centers;  // kSpheres: x, y, z per sphere ...
    std::vector<double> radii;   // ... and its radius
    std::vector<rmh::PrimDesc> prims;  // kPrims
    std::vector<rmh::NodeDesc> nodes;  // kNodes: the forest ...
    std::vector<int> roots;            // ... and its objects
};

// The three rings of launch_render.  Per-launch control slots: the 64 queue heads of a v2 launch, 256 bytes apart (rm_render_v2.hip RM_QUEUES, RM_QSTRIDE), and the
// accumulator block of the fused diagnostics (rm_diag.h).  Zeroed once, in init; every launch's last wave leaves its slots
// zeroed.  Beside a launch's heads, under the same slot number, the table of leaf screen rectangles its workgroups fill
// (option `rect_cull`; RM_RECT_CULL_MAX_LEAVES entries, written before they are read: never cleared).  A launch owns what it took until kLaunches - 1 later launches have taken theirs (frames in flight on several streams).
struct LaunchSlots {
    static constexpr unsigned kLaunches = 1024, kHeads = 64, kHeadWords = 64;
    unsigned int *heads = nullptr;  // [kLaunches][kHeads][kHeadWords]
    RmDiagBlock *blocks = nullptr;  // [kLaunches]
    RmLeafRect *rects = nullptr;    // [kLaunches][RM_RECT_CULL_MAX_LEAVES]
    unsigned int head_slot = 0, block_slot = 0;

    hipError_t init() {
        const size_t head_bytes = sizeof(unsigned int) * kLaunches * kHeads * kHeadWords, block_bytes = sizeof(RmDiagBlock) * kLaunches;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&heads), head_bytes);
        if (e == hipSuccess) e = hipMemset(heads, 0, head_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&blocks), block_bytes);
        if (e == hipSuccess) e = hipMemset(blocks, 0, block_bytes);
        return e == hipSuccess ? hipMalloc(reinterpret_cast<void **>(&rects), sizeof(RmLeafRect) * kLaunches * RM_RECT_CULL_MAX_LEAVES) : e;
    }
    void release() {
        (void)hipFree(heads);
        (void)hipFree(blocks);
        (void)hipFree(rects);
    }
    // the rectangle table that goes with the heads take_heads() handed out last
    RmLeafRect *rects_of_last_heads() { return rects && head_slot ? rects + static_cast<size_t>(RM_RECT_CULL_MAX_LEAVES) * ((head_slot - 1) % kLaunches) : nullptr; }
    unsigned int *take_heads() { return heads ? heads + static_cast<size_t>(kHeads) * kHeadWords * (head_slot++ % kLaunches) : nullptr; }
    RmDiagBlock *take_block() { return blocks ? blocks + block_slot++ % kLaunches : nullptr; }
};

// Who owns which entries of a ring that calls in flight share (FrameRing, CompareRing).  A call takes n consecutive entries, from
// the start again when the end is too near, and records an event behind its launch (launched).  The entries stay that call's
// until the event has completed: take() waits for the event of every earlier call whose entries overlap the ones it hands out,
// whatever stream that call ran on.  A call without an event (none to be had, or its launch failed) has its stream
// synchronised instead.  Batches of up to half the ring therefore never wait for the call just before them; larger ones do.
struct RingClaims {
    struct Claim {
        size_t first, n;
        hipEvent_t done;
    };
    size_t next = 0;
    std::vector<Claim> claims;  // calls whose event has not been waited for yet

    void retire_all() {  // (the device is idle)
        for (Claim &c : claims) (void)hipEventDestroy(c.done);
        claims.clear();
        next = 0;
    }
    // first entry of n <= cap consecutive ones that no call in flight owns
    hipError_t take(size_t n, size_t cap, size_t *first) {
        if (next + n > cap) next = 0;
        const size_t lo = next, hi = next + n;
        for (size_t k = 0; k < claims.size();) {
            const Claim c = claims[k];
            if (c.first < hi && lo < c.first + c.n) {
                const hipError_t e = hipEventSynchronize(c.done);
                if (e != hipSuccess) return e;
                (void)hipEventDestroy(c.done);
                claims.erase(claims.begin() + static_cast<std::ptrdiff_t>(k));
            } else ++k;
        }
        *first = lo;
        next = hi;
        return hipSuccess;
    }
    // behind the launch (or the failed attempt) that uses the entries of the last take
    void launched(size_t first, size_t n, hipStream_t stream) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, stream) == hipSuccess) {
            claims.push_back(Claim{first, n, ev});
            return;
        }
        if (ev) (void)hipEventDestroy(ev);
        (void)hipStreamSynchronize(stream);
    }
};

// The ring of rm_render_frames_device: per frame of a call one RmFrameView (the frame's camera and time; written by the host
// into a pinned mirror and copied on the call's stream) and one RmFrameDiagBlock (rm_diag.h; zeroed when allocated, left zeroed
// by the last wave of its frame).
//  - Entries are owned as RingClaims says -- mirror, table and blocks alike -- so neither the host (writing the mirror) nor a
//    later launch (adding into the blocks) meets a call in flight.
//  - Allocated at the first call, kFrames entries (5 MB).  A call of more frames replaces the ring by one that holds exactly
//    it: the device is synchronised first (nothing in flight reads the old ring), so that one call is not asynchronous.
struct FrameRing {
    static constexpr size_t kFrames = 4096;
    RmFrameView *host = nullptr, *dev = nullptr;
    RmFrameDiagBlock *blocks = nullptr;
    size_t cap = 0;
    RingClaims owners;

    void release() {
        owners.retire_all();
        (void)hipHostFree(host);
        (void)hipFree(dev);
        (void)hipFree(blocks);
        host = dev = nullptr;
        blocks = nullptr;
        cap = 0;
    }
    hipError_t take(size_t n, size_t *first) {
        if (n > cap) {
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return e;
            release();
            const size_t want = n > kFrames ? n : kFrames;
            e = hipHostMalloc(reinterpret_cast<void **>(&host), want * sizeof(RmFrameView), hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&dev), want * sizeof(RmFrameView));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&blocks), want * sizeof(RmFrameDiagBlock));
            if (e == hipSuccess) e = hipMemset(blocks, 0, want * sizeof(RmFrameDiagBlock));
            if (e != hipSuccess) {
                release();
                return e;
            }
            cap = want;
        }
        return owners.take(n, cap, first);
    }
    void launched(size_t first, size_t n, hipStream_t stream) { owners.launched(first, n, stream); }
};

// The ring of rm_compare_frames_device: what the workgroups of a frame hand to the one that writes the frame's record
// (compare_kernel, rm_frame_ops.hip) -- one RmComparePartial per workgroup and, at the index of the frame's first workgroup, the
// frame's ticket counter (zeroed when allocated, left at zero by the workgroup that took the last ticket; partial records are
// overwritten whole, never cleared).  Only frames of more than one workgroup use it, and a launch has at most 2 048 workgroups
// in such frames (rm_compare_blocks_per_frame): kEntries is never too small.  Allocated at the first call that needs it (544 KB);
// entries are owned as RingClaims says.
struct CompareRing {
    static constexpr size_t kEntries = 4096;
    RmComparePartial *partials = nullptr;
    unsigned int *counters = nullptr;
    RingClaims owners;

    void release() {
        owners.retire_all();
        (void)hipFree(partials);
        (void)hipFree(counters);
        partials = nullptr;
        counters = nullptr;
    }
    hipError_t take(size_t n, size_t *first) {
        if (n > kEntries) return hipErrorInvalidValue;
        if (!partials) {
            hipError_t e = hipMalloc(reinterpret_cast<void **>(&partials), kEntries * sizeof(RmComparePartial));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&counters), kEntries * sizeof(unsigned int));
            if (e == hipSuccess) e = hipMemset(counters, 0, kEntries * sizeof(unsigned int));
            if (e != hipSuccess) {
                release();
                return e;
            }
        }
        return owners.take(n, kEntries, first);
    }
    void launched(size_t first, size_t n, hipStream_t stream) { owners.launched(first, n, stream); }
};

// The ring of rm_counter_hist_device: per frame of more than one workgroup one RmHistScratch (2 096 bytes: the frame's scratch
// histograms, sums, extremes and ticket counter; zeroed when allocated, left all zero by the workgroup that took the last ticket --
// hist_kernel, rm_frame_ops.hip).  A launch has at most 2 048 workgroups in such frames (rm_compare_blocks_per_frame), so at most
// 1 024 such frames: no call needs more than half of kEntries.  Allocated at the first call that needs it (4.2 MB); entries are
// owned as RingClaims says.
struct HistRing {
    static constexpr size_t kEntries = 2048;
    RmHistScratch *entries = nullptr;
    RingClaims owners;

    void release() {
        owners.retire_all();
        (void)hipFree(entries);
        entries = nullptr;
    }
    hipError_t take(size_t n, size_t *first) {
        if (n > kEntries) return hipErrorInvalidValue;
        if (!entries) {
            hipError_t e = hipMalloc(reinterpret_cast<void **>(&entries), kEntries * sizeof(RmHistScratch));
            if (e == hipSuccess) e = hipMemset(entries, 0, kEntries * sizeof(RmHistScratch));
            if (e != hipSuccess) {
                release();
                return e;
            }
        }
        return owners.take(n, kEntries, first);
    }
    void launched(size_t first, size_t n, hipStream_t stream) { owners.launched(first, n, stream); }
};

// The LPT ring (option `lpt`; rm_render_v2.hip, lpt_sort_kernel): a v2 launch sorts its items longest-first from the costs the
// previous launch recorded, into a permutation of its own, and records its own costs; one slot per launch in flight.
//  - The buffers are allocated at the first acquire; both exist or neither does (launches then keep their queues' order).
//  - The costs are per item of THIS tiling of THIS row set: cost_prev is given only when the previous launch had the same
//    geometry key; any change restarts the feedback (costs read as zero).
//  - A slot is reused once the launch that owned it is over: acquire waits for the event launched() recorded (16 launches ago).
//  - acquire advances the launch counter whether or not the launch then succeeds.
struct LptRing {
    static constexpr int kSlots = 16;
    static constexpr int kQueues = 64;    // rm_render_v2.hip RM_QUEUES
    static constexpr int kStride = 4096;  // items per queue; larger frames render without LPT
    static constexpr size_t kPerSlot = static_cast<size_t>(kQueues) * kStride;
    uint8_t *cost = nullptr;   // [kSlots][kPerSlot]
    uint16_t *perm = nullptr;  // [kSlots][kPerSlot]
    unsigned int launches = 0;
    long long geometry = -1;
    hipEvent_t done[kSlots] = {};

    unsigned last() const { return (launches + kSlots - 1) % kSlots; }  // the slot the last launch took
    const uint8_t *last_costs() const { return cost && launches ? cost + last() * kPerSlot : nullptr; }  // rm_debug_read_lpt_costs

    // the launch geometry of p -> p.lpt_cost_prev, lpt_cost_out, lpt_perm_out, lpt_stride (left null / zero without buffers)
    void acquire(RmRenderParams &p) {
        if (!cost && (hipMalloc(reinterpret_cast<void **>(&cost), kSlots * kPerSlot) != hipSuccess ||
                      hipMalloc(reinterpret_cast<void **>(&perm), kSlots * kPerSlot * sizeof(uint16_t)) != hipSuccess)) {
            (void)hipFree(cost);
            cost = nullptr;
            perm = nullptr;
        }
        if (!cost) return;
        const long long geom = ((static_cast<long long>(p.width) * 65536 + p.local_rows) * 1024 + p.tile_w) * 1024 + p.item_px + (p.item_wide ? 512 : 0) +
                               (p.stripe_rows ? (1ll << 62) + p.part * 131 + p.n_parts : 0) + p.y_start * 7919ll;
        const unsigned slot = launches % kSlots, prev = last();
        const bool have_prev = launches > 0 && geom == geometry;
        geometry = geom;
        launches++;
        if (done[slot]) (void)hipEventSynchronize(done[slot]);
        p.lpt_stride = kStride;
        p.lpt_cost_prev = have_prev ? cost + prev * kPerSlot : nullptr;
        p.lpt_cost_out = cost + slot * kPerSlot;
        p.lpt_perm_out = perm + slot * kPerSlot;
    }
    void launched(hipStream_t stream) {  // behind a launch that succeeded with the slot of acquire
        hipEvent_t &ev = done[last()];
        if (!ev) (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (ev) (void)hipEventRecord(ev, stream);
    }
    void release() {
        (void)hipFree(cost);
        (void)hipFree(perm);
        for (hipEvent_t ev : done)
            if (ev) (void)hipEventDestroy(ev);
    }
};

// The octree camera-table ring (render_kernel_oct): the octree relative to a camera position (RmOctFrameNode), one table per
// position, shared by every launch with that position (frames in flight with one camera build it once) and rewritten only
// when the ring comes round.
//  - acquire tries the current table first, then all kSlots.  A table matches when it is valid, of this scene generation,
//    and its three origin doubles are equal.
//  - A table found may still be under construction on the stream that first saw the position: a launch on another stream
//    that has not read it before (one that has is ordered behind the builder already) waits for the `built` event; without
//    an event, or if the wait fails, it synchronises the builder's stream.  (the `users` events only made the
//    next WRITER wait for the readers, never a reader for the writer.)
//  - A new position takes slot next++ % kSlots: every reader event of the slot is waited for and destroyed and `users`
//    cleared (it lists the readers of THIS table).  The memory is reallocated only when the node count grew.  The table is
//    built on the launch's stream with `built` recorded right behind it; failing that the stream is synchronised.
//  - A failed allocation or table launch yields null: the launcher then takes render_kernel<1, false, 0>.
//  - read_by, behind the render launch whether or not it succeeded, records the stream's reader event: whoever rewrites the
//    table waits for this launch.  No event to be had: the stream is synchronised.
struct OctTableRing {
    struct Table {
        double origin[3] = {0, 0, 0};
        unsigned long long gen = 0;
        bool valid = false;
        RmOctFrameNode *dev = nullptr;
        size_t nodes = 0;
        std::vector<std::pair<hipStream_t, hipEvent_t>> users;
        hipStream_t builder = nullptr;  // the stream oct_frame_table_kernel ran on
        hipEvent_t built = nullptr;
    };
    static constexpr int kSlots = 32;
    Table slots[kSlots];
    unsigned next = 0;
    int cur = -1;

    Table *acquire(unsigned long long gen, const RmOctNode *oct, int32_t oct_nodes, const double origin[3], hipStream_t stream) {
        auto matches = [&](const Table &t) {
            return t.valid && t.gen == gen && t.origin[0] == origin[0] && t.origin[1] == origin[1] && t.origin[2] == origin[2];
        };
        Table *found = cur >= 0 && matches(slots[cur]) ? &slots[cur] : nullptr;
        for (int k = 0; !found && k < kSlots; ++k)
            if (matches(slots[k])) {
                found = &slots[k];
                cur = k;
            }
        if (found) {
            bool seen = found->builder == stream;
            for (auto &u : found->users) seen = seen || u.first == stream;
            if (!seen && (!found->built || hipStreamWaitEvent(stream, found->built, 0) != hipSuccess)) (void)hipStreamSynchronize(found->builder);
            return found;
        }
        const int k = static_cast<int>(next++ % kSlots);
        Table &t = slots[k];
        for (auto &u : t.users) {
            (void)hipEventSynchronize(u.second);
            (void)hipEventDestroy(u.second);
        }
        t.users.clear();
        t.valid = false;
        const size_t n = static_cast<size_t>(oct_nodes);
        if (t.nodes < n) {
            (void)hipFree(t.dev);
            t.dev = nullptr;
            t.nodes = 0;
            if (hipMalloc(reinterpret_cast<void **>(&t.dev), n * sizeof(RmOctFrameNode)) == hipSuccess) t.nodes = n;
            else (void)hipGetLastError();
        }
        if (!t.dev || rm_launch_oct_frame_table(oct, oct_nodes, origin, t.dev, stream) != hipSuccess) return nullptr;
        for (int a = 0; a < 3; ++a) t.origin[a] = origin[a];
        t.gen = gen;
        t.valid = true;
        t.builder = stream;
        if (!t.built && hipEventCreateWithFlags(&t.built, hipEventDisableTiming) != hipSuccess) t.built = nullptr;
        if (!t.built || hipEventRecord(t.built, stream) != hipSuccess) (void)hipStreamSynchronize(stream);
        cur = k;
        return &t;
    }
    static void read_by(Table &t, hipStream_t stream) {
        hipEvent_t ev = nullptr;
        for (auto &u : t.users)
            if (u.first == stream) ev = u.second;
        if (!ev) {
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) t.users.emplace_back(stream, ev);
            else ev = nullptr;
        }
        if (ev) (void)hipEventRecord(ev, stream);
        else (void)hipStreamSynchronize(stream);
    }
    void release() {
        for (Table &t : slots) {
            (void)hipFree(t.dev);
            for (auto &u : t.users) (void)hipEventDestroy(u.second);
            if (t.built) (void)hipEventDestroy(t.built);
        }
    }
};

}  // namespace

struct rm_ctx {
    int device = -1;
    bool has_device = false;
    std::string err = "";
    hipStream_t stream = nullptr;  // for the host-buffer entry points

    bool have_scene = false;
    bool scene_is_uploaded = false;  // active scene came from rm_scene_from_spheres
    int scene_preset = 0;
    rmh::HostScene host;
    DeviceScene dev;

    bool have_uploaded = false;
    SceneDesc uploaded;  // the last rm_scene_from_spheres / _prims / _nodes upload, kept for accel changes by later jobs
    double time = 0.0;  // Scene.updateTime: the last job's time, or rm_scene_set_time

    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    hipEvent_t scratch_busy = nullptr;  // behind the last launches that read the scratch after their entry returned (Staging::keep)
    RmDiagDevice *d_diag = nullptr;
    float light[3] = {0, 0, 0};

    int64_t opt_tile_w = 8;  // 8 x 8-pixel batches (a frame alone, round 3: 128-pixel items of 8 x 16: 1.09 ms; of 16 x 8: 1.17 ms)
    bool tile_w_set = false;  // the tile_w option was set: the value then holds for every kernel (else v1 kernels use 8 x 8 wave tiles)
    int64_t opt_filter = 1;
    int64_t opt_lds = 1;
    int64_t opt_kernel = 0;  // 0 = auto: v2 for BVH / no acceleration, v1 for the octree (its lean kernel for sphere scenes: opt_oct_lean) and small scenes
    int64_t opt_list_cap = 32;
    int64_t opt_coop = 1;
    int64_t opt_grid = 1;
    int64_t opt_nn = 2;  // per-cell nearest-candidate lists for the all-primitive fallback: 0 off, 1 on, 2 auto (scenes of
                         // <= 512 spheres, where the 48^3 candidate grid keeps the lists short: C3 2.65 -> 2.62 ms)
    int64_t opt_ext = 1;  // the exterior candidate grid serves the all-primitive evaluations outside the BVH root box (rm_scene_host.cpp build_exterior_grid)
    int64_t opt_blocks_per_cu = 6;  // persistent workgroups per launch and CU: what the kernel's 80 VGPRs and 26 KB of LDS allow (a frame alone, round 3: 4: 1.42 ms, 6: 1.32, 7: 1.30)
    int64_t opt_lds_fill = 0;
    // v2: a persistent launch brings at least ceil(RM_V2_WAVES / hw_queues) workgroups per CU (launch_fill below).  Launches on
    // streams that share a hardware queue run one after the other, so a launch never overlaps with more launches than the
    // process has queues: with HIP's default of four, launches of one workgroup per CU fill four of a SIMD's six wave slots
    // whatever the caller keeps in flight.  0: bring exactly blocks_per_cu (measurement sweeps).
    int64_t opt_min_fill = 1;
    // v2, above that floor: the floor counts on Q launches overlapping, and with more streams than queues they do not (the short
    // queues drain first: overlap_fill below).  A launch whose work items pay for it brings what fills the CU at the overlap
    // that is really there.  0: the floor alone.
    int64_t opt_overlap_fill = 1;
    int hw_queues = 4;  // GPU_MAX_HW_QUEUES as rm_create found it (read_hw_queues); the library never sets it
    uint32_t last_v2_shape[7] = {0, 0, 0, 0, 0, 0, 0};  // the last v2 launch: workgroups, threads per workgroup, dynamic LDS bytes (rm_debug_last_launch); whether section M
                                                  // tested its steps against the step-box table (rm_debug_step_box); whether its cull went by leaf rectangles (rm_debug_rect_cull);
                                                  // whether section B read its candidates from the cell table (rm_debug_cell_tab); whether section M bounded the
                                                  // runner-up by its own distance (rm_debug_runner_up)
    int64_t opt_item_wide = 0;  // v2: the 64-pixel batches of an item side by side (1) or one above the other (0)
    int64_t opt_multi_step = 1;  // v2 BVH: in-round march steps (rm_render_v2.hip, section M)
    int64_t opt_step_box = 1;    // ... test their leaf sets against the bracket of the round's point in the scene's threshold tables (rm_scene_host.cpp
                                 // build_step_box) where the scene has them and they fit the launch's LDS; 0: the exact test against the leaf lists
    int64_t opt_cell_tab = 1;    // v2 BVH: section B reads a point's candidate spheres, and section M its step box, from the scene's table of threshold cells
                                 // (rm_scene_host.cpp build_cell_tab) where the launch takes the step-box table and the cell table fits the LDS the point-query grid frees
    int64_t opt_runner_up = 1;   // v2 BVH, one-radius launches with the cell table: section M bounds the runner-up sphere by its own distance at the new point and
                                 // the candidates behind it by the third scan key's bound (round 12: fewer runs end, fewer rounds begin); 0: all of them by lb2 - dd
    int64_t opt_lds_kb = 0;         // v2: LDS budget per workgroup the launcher trims the hit lists to (0: as many workgroups per CU as the kernel's registers allow; 32: five per CU, 40: four)
    int64_t opt_refill = 64;
    int64_t opt_recs = 1;  // octree leaves read leaf-ordered sphere records
    int64_t opt_static = 0;  // accepted and ignored since round 3 (a static share of every tile queue, overtaken in round 2; the 64 queue heads of round 3 removed its reason)
    int64_t opt_lut = 1;   // Octree.findNode through the 64^3 cell table
    int64_t opt_cull = 1;     // v2: whole 64-pixel batches find their hit leaves by a bundle-frustum cull instead of the tree walk
    // v2, with `cull`: the cull compares the batch's pixel rectangle with a per-launch table of leaf screen rectangles instead of
    // working four planes out per batch and leaf (rm_kernels.h rm_leaf_rect; scenes of up to RM_RECT_CULL_MAX_LEAVES leaves,
    // cameras rm_rect_cull_camera_ok admits), and a batch without a candidate sets up no ray; 0: the plane cull
    int64_t opt_rect_cull = 1;
    std::vector<uint16_t> cull_leaves;  // cull_leaf_table of the active scene (what DeviceScene::bvh_leaves holds; kept for contexts without a device)
    int64_t opt_rel = 1;      // v2: BVH node boxes relative to the frame's ray origin, as doubles in LDS (slab test without conversions)
    int64_t opt_uniform = 1;  // v2: scenes whose spheres all have one radius rank candidates by squared centre distance
    int64_t opt_sub = 1;   // crowded octree leaves scan their sub-cell candidate lists
    int64_t opt_hw_xcd = 1;
    int64_t opt_v1_lists = 1;  // v1 BVH kernels: per-ray hit-leaf lists instead of one tree walk per interval advance
    int64_t opt_v1_block = 64;  // v1 kernels: threads per workgroup (one wave: wave slots refill one by one)
    int64_t opt_oct_lean = 1;  // octree, sphere scenes, sphere tracer: render_kernel_oct (rm_kernels.hip) instead of render_kernel<1, false, 0>
    int64_t opt_lpt = 1;  // v2: longest-first item order from the previous frame's item durations (shortens the tail of a frame that runs alone: 1.13 -> 1.08 ms)
    LaunchSlots slots;        // the three rings of launch_render (above)
    LptRing lpt;
    OctTableRing oct_tables;
    FrameRing frames;         // rm_render_frames_device
    CompareRing compare;      // rm_compare_frames_device
    HistRing hists;           // rm_counter_hist_device
    unsigned long long scene_gen = 0;  // bumped by every upload_scene
    int64_t opt_n0_batch = 64;  // v2 BVH: see RmRenderParams::n0_batch
    int64_t opt_length = 0;  // vec3.length: 0 Math.hypot (gl-matrix 3.0 - 3.4.3), 1 Math.sqrt(x*x + y*y + z*z)
    // Point, field, tile and mesh queries answer from the exact field E(x) = min(10, min over ALL objects of Primitive.sdf(x))
    // instead of Scene.getDistance (include/rm_raymarch.h, "the exact field").  What they walk (ensure_exact_tree): the scene's
    // BVH, or -- octree and None scenes -- the exact tree below, built at the first exact query after the scene was made and
    // dropped by every upload_scene.
    int64_t opt_exact = 0;
    bool exact_ready = false;  // exact_mode and exact_tree are the active scene's
    int exact_mode = 0;        // rmh::exact_tree_mode, or 0 where the own tree could not be built
    rmh::ExactTree exact_tree; // mode 2
    RmBvhNode *d_exact_nodes = nullptr;  // mode 2 on a context with a device
    int32_t *d_exact_ids = nullptr;
    const char *last_kernel = "";
    std::string last_kernel_kept;  // rm_scene_edit_spheres: the name behind last_kernel across the upload (which releases run-time compiled kernels and their names)
    // rm_scene_edit_spheres: the four pair loops of the scene build (rm_scene_host.h, PairLoops) run on the device
    // (rm_scene_build.hip); 0: the host builder for everything.  The upload entries never read it.
    int64_t opt_device_build = 1;
    // Expression forests: the scene's programs compiled into the one-ray-per-lane kernels at run time (rm_rtc.h; option
    // `specialise`, default on).  One kernel per (acceleration structure, marcher family, vec3.length form) the scene is
    // rendered with, compiled at its first launch (1.5 - 3 s, synchronous) and kept until the scene is replaced.  A compile
    // that fails, or whose kernel spills a VGPR (refused: rm_rtc.h), is remembered with its log (rm_rtc_status) and the
    // interpreter of rm_program.h serves the scene.
    int64_t opt_specialise = 1;
    // sphere lists of fewer spheres than this run in the one-ray-per-lane kernels as the scene's own code (C2, nine spheres at
    // 1080p: 0.22 ms alone against 0.32 in the v2 wave loop, 8 780 against 8 340 frames/s in flight); without hiprtc the rule is < 8
    int64_t opt_rtc_spheres = 16;
    int64_t opt_prune = 1;  // specialised kernels: exact pruning of smooth unions / subtractions (rm_rtc.cpp); takes effect at the next scene build
    std::string rtc_src;
    std::map<int, rmrtc::Kernel> rtc_kernels;   // handles; the modules belong to rm_rtc's process-wide cache ...
    std::vector<rmrtc::Kernel> rtc_owned;       // ... except these (compiled while the cache was full)
    std::map<int, std::string> rtc_failed;
    std::string rtc_log;  // of the most recent compile
    // The v2 wave loop compiled for a launch configuration that keeps coming back (rm_v2_fields.h, rm_rtc_v2_hook below): after
    // `specialise_v2_after` launches with the same configuration (default 3; 0: never) the kernel is compiled with that
    // configuration's parameters as literals (~2 s; synchronous with `specialise` = 1, in the background with 2) and used from
    // then on.  Keyed by a hash of the configuration; the modules live in rm_rtc's process-wide cache.
    struct V2Special {
        int launches = 0;
        int state = 0;  // 0 counting, 2 compiling in the background, 1 ready, -1 failed
        bool lite = false;  // the first compile (with the scene's counts as literals) was refused: without them
        rmrtc::Kernel k;
    };
    std::unordered_map<uint64_t, V2Special> v2_special;
    int64_t opt_v2_after = 3;
    // small host tables the sharded entry points need on the device (stripe lists, stripe -> source maps): cached by
    // content, each in its own allocation, so a table a launch in flight still reads is never overwritten
    struct DevTable {
        std::vector<int32_t> host;
        int32_t *dev = nullptr;
    };
    std::vector<DevTable> tables;
    int64_t opt_item_px = 128;  // two 64-pixel batches per queue claim: 7-10 % faster than 64 at the end of round 1, 256 loses
    void *diag_next = nullptr;  // rm_render_attach_diagnostics, one-shot
    unsigned long long *d_stamps = nullptr;  // diagnostic build only
    int num_cus = 256;
};

namespace {

int fail(rm_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return code;
}

int hip_fail(rm_ctx *ctx, hipError_t e, const char *what) {
    return fail(ctx, RM_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The hardware queues the HIP runtime of this process opens: GPU_MAX_HW_QUEUES when it is a decimal integer >= 1, else 4 (HIP's
// default: unset, empty, not a number, <= 0).  Read, never set: the count is the host's to choose.
int read_hw_queues() {
    const char *s = std::getenv("GPU_MAX_HW_QUEUES");
    if (!s || !*s) return 4;
    char *end = nullptr;
    errno = 0;
    const long long v = std::strtoll(s, &end, 10);
    if (errno || end == s || *end != '\0' || v <= 0) return 4;
    return static_cast<int>(std::min<long long>(v, INT_MAX));
}

// Workgroups per CU a persistent v2 launch brings when the caller asked for `asked` (option `blocks_per_cu`).  At most
// `queues` launches run at once, and a CU holds RM_V2_WAVES of the wave loop's workgroups: a launch that brings fewer than
// ceil(RM_V2_WAVES / queues) leaves wave slots empty whatever the caller overlaps.  Q = 4: 2; Q >= 6: 1 (as asked); Q = 1, 2, 3: 6, 3, 2.
int launch_fill(int asked, int queues, bool min_fill) {
    if (!min_fill) return asked;
    const int q = queues > 0 ? queues : 4;
    return std::max(asked, (RM_V2_WAVES + q - 1) / q);
}

// The workgroups per CU a v2 launch brings where its frame can pay for them (rm_v2_overlap_per_cu, rm_kernels.h), else the
// floor above.  The floor fills a CU while all Q queues run a launch; streams are not dealt evenly over the queues, so for part
// of every burst fewer run.  A kernel trace of twelve streams on four queues (profiles/NOTES.md, round 6) has fewer than four
// launches running for 53 % of the busy time, 1.74 of them on average: E(Q) = 0.436 Q launches overlap while the short queues
// are drained, and a launch brings ceil(RM_V2_WAVES / E(Q)), at most RM_V2_WAVES.  Q = 4 (measured): 4.  Q = 1, 2, 3, 5
// (extrapolated with the same share): 6, 6, 5, 3.  Q >= RM_V2_WAVES: the floor, as asked.
int overlap_fill(int asked, int queues, bool min_fill, bool overlap) {
    const int floor = launch_fill(asked, queues, min_fill);
    const int q = queues > 0 ? queues : 4;
    if (!min_fill || !overlap || q >= RM_V2_WAVES) return floor;
    const int per_mille = 436 * q;  // 1000 E(Q)
    return std::max(floor, std::min(RM_V2_WAVES, (RM_V2_WAVES * 1000 + per_mille - 1) / per_mille));
}

// A kernel compiled at run time (rm_rtc.h), as `specialise` says: 1 waits for the compile; 2 never waits -- the ahead-of-time
// kernels render until the background compile has finished.  1: k is set; 0: still compiling; -1: failed or refused.  The
// compiler's log goes to ctx->rtc_log either way.
int obtain_kernel(rm_ctx *ctx, const std::string &src, int accel, bool other, bool length_sqrt, rmrtc::Kernel &k) {
    if (ctx->opt_specialise == 2) return rmrtc::compile_async(ctx->device, src, accel, other, length_sqrt, k, ctx->rtc_log);
    bool cached = false;
    if (!rmrtc::compile_cached(ctx->device, src, accel, other, length_sqrt, k, ctx->rtc_log, &cached)) return -1;
    if (!cached) ctx->rtc_owned.push_back(k);  // the process-wide cache is full: this context unloads the module with the scene
    return 1;
}

// the kernels exist twice: vec3.length = Math.hypot, and = sqrt(x*x + y*y + z*z) (rm_kernels.h, option `length`)
// the scene's specialised kernel for (accel, marcher family, length form), compiled on first use; nullptr: the interpreter serves
const rmrtc::Kernel *specialised_kernel(rm_ctx *ctx, int accel, bool other) {
    if (!ctx->opt_specialise || ctx->rtc_src.empty() || !ctx->has_device) return nullptr;
    const int key = (accel * 2 + (other ? 1 : 0)) * 2 + (ctx->opt_length ? 1 : 0);
    auto it = ctx->rtc_kernels.find(key);
    if (it != ctx->rtc_kernels.end()) return &it->second;
    if (ctx->rtc_failed.count(key)) return nullptr;
    rmrtc::Kernel k;
    const int st = obtain_kernel(ctx, ctx->rtc_src, accel, other, ctx->opt_length != 0, k);
    if (st < 0) ctx->rtc_failed[key] = ctx->rtc_log;
    if (st <= 0) return nullptr;
    return &(ctx->rtc_kernels[key] = k);
}

}  // namespace

const void *rm_rtc_v2_hook(const RmRenderParams &p, int accel, bool lds, bool ur, bool rel, bool length_sqrt) {
    rm_ctx *ctx = static_cast<rm_ctx *>(p.rtc_ctx);
    if (!ctx || !ctx->opt_specialise || ctx->opt_v2_after <= 0) return nullptr;
    const int bits = (accel & 3) | (lds ? 4 : 0) | (ur ? 8 : 0) | (rel ? 16 : 0) | rmrtc::kV2Bit;
    rm_ctx::V2Special &e = ctx->v2_special[rmrtc::v2_fixed_hash(p, bits | (length_sqrt ? 512 : 0))];
    if (e.state == 1) return e.k.render;
    if (e.state < 0) return nullptr;
    if (e.state == 0 && ++e.launches < ctx->opt_v2_after) return nullptr;
    // with the scene's counts as literals first; a kernel refused for spilling (small scenes: their loops unroll) once more without.
    // Either form, when refused as the compiler's defaults make it, once more without machine-level hoisting (rm_rtc.cpp compile_v2).
    for (;;) {
        int st = obtain_kernel(ctx, rmrtc::v2_fixed_source(p, !e.lite), bits, false, length_sqrt, e.k);
        if (st < 0) st = obtain_kernel(ctx, rmrtc::v2_fixed_source(p, !e.lite), bits | rmrtc::kV2NoLicmBit, false, length_sqrt, e.k);
        e.state = st > 0 ? 1 : (st < 0 ? -1 : 2);
        if (st >= 0 || e.lite) break;
        e.lite = true;
        e.state = 0;
    }
    return e.state == 1 ? e.k.render : nullptr;
}

namespace {

// diag_out: the accumulator rm_render_attach_diagnostics attached to this call (render_device took it), or null
hipError_t launch_render(rm_ctx *ctx, const RmRenderParams &p_in, RmDiagDevice *diag_out, hipStream_t stream) {
    RmRenderParams p = p_in;
#if !defined(RM_STAMPS) && !defined(RM_COUNTS) && !defined(RM_STAMPS_LOG) && !defined(RM_STAMPS_CLAIM)  // (diagnostic builds keep their instrumented kernels)
    p.rtc_ctx = ctx;
#endif
    const bool empty = p.local_rows <= 0 || p.width <= 0;  // a launch without pixels runs no kernel
    const bool v2 = p.variant == 2 && p.algorithm == 0;
    // every launch of the one-ray-per-lane kernels (not the v2 wave loop, not the lean octree kernel) takes the scene's own kernel if it has one
    const bool lean_oct = p.accel == 1 && p.oct_lean && !p.general && p.algorithm == 0 && p.oct_lut && p.oct_recs && p.filter;
    const rmrtc::Kernel *special = v2 || lean_oct ? nullptr : specialised_kernel(ctx, p.accel, p.algorithm != 0);
    p.rtc_function = special ? special->render : nullptr;
    OctTableRing::Table *oct_table = lean_oct ? ctx->oct_tables.acquire(ctx->scene_gen, p.oct, p.oct_nodes, p.origin_d, stream) : nullptr;
    p.oct_frame = oct_table ? oct_table->dev : nullptr;  // null: the launcher takes render_kernel<1, false, 0>
    if (ctx->opt_lpt && v2) ctx->lpt.acquire(p);  // longest-first item order
    if (v2 && !empty) p.tile_counters = ctx->slots.take_heads();
    p.leaf_rects = v2 && !empty && p.rect_cull ? ctx->slots.rects_of_last_heads() : nullptr;
    if (!p.leaf_rects) p.rect_cull = 0;
    // Fused diagnostics (rm_render_attach_diagnostics).  v2 launches always get an accumulator block: their last
    // wave also re-zeroes the launch's queue heads.  A launch without pixels writes the neutral elements.
    p.diag_out = diag_out;
    // The one-ray-per-lane kernels run one-wave workgroups: 129 600 waves per 4K frame, each of which would end with five
    // device-scope atomics and a wait for four of them.  Measured (round 3, frames in flight): Pyramid of Boxes 1 348 frames/s
    // with that epilogue against 1 561 with the two reduction launches over the stored counters, C5 493 against 512.  So
    // when the call stores both counter buffers the diagnostics of a v1 launch come from rm_launch_reduce behind it (still one
    // call for the host, no host synchronisation); the in-kernel epilogue serves the calls that store no counters.
    RmDiagDevice *reduce_after = nullptr;
    if (p.diag_out && !v2 && !empty && p.sdf && p.iters) {
        reduce_after = p.diag_out;
        p.diag_out = nullptr;
    }
    p.diag_block = !empty && (p.diag_out || v2) ? ctx->slots.take_block() : nullptr;
    if (p.diag_out && empty) {
        const hipError_t ei = rm_launch_reduce_init(p.diag_out, stream);
        if (ei != hipSuccess) return ei;
    }
    hipError_t e = ctx->opt_length ? rm_launch_render_sqrt(p, stream, &ctx->last_kernel, ctx->last_v2_shape)
                                   : rm_launch_render(p, stream, &ctx->last_kernel, ctx->last_v2_shape);
    if (special && !empty) ctx->last_kernel = special->name.c_str();
    if (e == hipSuccess && reduce_after) {
        e = rm_launch_reduce_init(reduce_after, stream);
        if (e == hipSuccess) e = rm_launch_reduce(p.sdf, p.iters, static_cast<int64_t>(p.local_rows) * p.width, reduce_after, stream);
    }
    if (oct_table) OctTableRing::read_by(*oct_table, stream);
    if (e == hipSuccess && p.lpt_perm_out) ctx->lpt.launched(stream);
    return e;
}

#define RM_HIP(ctx, call)                                       \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
    } while (0)

// The preamble of an entry that needs a device: a null context is RM_E_INVALID (there is no context to leave a text in), a
// host-only one RM_E_NO_DEVICE with `text`.  hipSetDevice is not part of it: in all but the rm_debug_read_* entries argument
// checks stand between the two, and the order of checks is behaviour.
#define RM_NEED_DEVICE(ctx, text)                                             \
    do {                                                                      \
        if (!(ctx)) return RM_E_INVALID;                                      \
        if (!(ctx)->has_device) return fail(ctx, RM_E_NO_DEVICE, text);       \
    } while (0)

void free_device_scene(rm_ctx *ctx) {
    for (auto &k : ctx->rtc_owned) rmrtc::release(k);  // (callers have synchronised the device)
    ctx->rtc_owned.clear();
    ctx->rtc_kernels.clear();
    ctx->v2_special.clear();  // (a new scene is a new configuration anyway: its counts and LDS layout are in the key)
    ctx->rtc_failed.clear();
    ctx->last_kernel = "";
    ctx->exact_ready = false;  // the exact tree is the old scene's: the next exact query builds the new one's
    ctx->exact_mode = 0;
    ctx->exact_tree = rmh::ExactTree();
    if (!ctx->has_device) return;
    (void)hipFree(ctx->d_exact_nodes);
    (void)hipFree(ctx->d_exact_ids);
    ctx->d_exact_nodes = nullptr;
    ctx->d_exact_ids = nullptr;
    DeviceScene &d = ctx->dev;
#define RM_X(name, always) (void)hipFree(d.name);
    RM_SCENE_ARRAYS(RM_X)
#undef RM_X
    (void)hipFree(d.bvh_leaves);
    d = DeviceScene();
}

// device copy of a small host table, cached by content (see rm_ctx::tables)
int device_table(rm_ctx *ctx, const int32_t *host, size_t n, const int32_t **out) {
    for (auto &t : ctx->tables)
        if (t.host.size() == n && std::memcmp(t.host.data(), host, n * sizeof(int32_t)) == 0) {
            *out = t.dev;
            return RM_OK;
        }
    if (ctx->tables.size() >= 256) {  // far more than any run deals; start over rather than grow without bound
        RM_HIP(ctx, hipDeviceSynchronize());
        for (auto &t : ctx->tables) (void)hipFree(t.dev);
        ctx->tables.clear();
    }
    rm_ctx::DevTable t;
    t.host.assign(host, host + n);
    RM_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&t.dev), (n ? n : 1) * sizeof(int32_t)));
    if (n) RM_HIP(ctx, hipMemcpy(t.dev, host, n * sizeof(int32_t), hipMemcpyHostToDevice));
    *out = t.dev;
    ctx->tables.push_back(std::move(t));
    return RM_OK;
}

template <typename T>
int upload_vec(rm_ctx *ctx, const std::vector<T> &v, T **out) {
    *out = nullptr;
    const size_t bytes = (v.empty() ? 1 : v.size()) * sizeof(T);
    RM_HIP(ctx, hipMalloc(reinterpret_cast<void **>(out), bytes));
    if (!v.empty()) RM_HIP(ctx, hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return RM_OK;
}

// Leaf table of the bundle cull (rm_render_v2.hip, bvh_prologue_cull): the node indices of the non-empty leaves, or none
// when the cull cannot serve this tree.  The cull tests leaves directly, which equals the reference's traversal only if a
// hit leaf implies hit ancestors: every box must lie inside its parent's, bit for bit (the builder takes unions, so it
// does; verified here rather than assumed).
std::vector<uint16_t> cull_leaf_table(const std::vector<RmBvhNode> &bvh) {
    std::vector<uint16_t> leaves;
    bool ok = !bvh.empty() && bvh.size() < 65536;
    std::vector<int> parent(bvh.size(), -1);
    for (size_t i = 0; ok && i < bvh.size(); ++i) {
        if (bvh[i].leaf >= 0) continue;
        for (size_t c = i + 1; c < static_cast<size_t>(bvh[i].skip) && c < bvh.size(); c = static_cast<size_t>(bvh[c].skip)) {
            parent[c] = static_cast<int>(i);
            if (bvh[c].skip <= static_cast<int>(c)) { ok = false; break; }
        }
    }
    for (size_t i = 0; ok && i < bvh.size(); ++i) {
        if (parent[i] >= 0)
            for (int k = 0; k < 3; ++k)
                if (!(bvh[i].lo[k] >= bvh[parent[i]].lo[k] && bvh[i].hi[k] <= bvh[parent[i]].hi[k])) ok = false;
        for (int k = 0; k < 3; ++k)  // a negative radius gives lo > hi: the slab test then is not monotone in the box
            if (!(bvh[i].lo[k] <= bvh[i].hi[k])) ok = false;
        if (i > 0 && parent[i] < 0) ok = false;  // not reached through the skip links: unknown shape
        if (bvh[i].leaf >= 0 && (bvh[i].leaf & 0xFF) > 0) leaves.push_back(static_cast<uint16_t>(i));
    }
    if (!ok || leaves.size() > 256) leaves.clear();
    return leaves;
}

int upload_scene(rm_ctx *ctx) {
    // Scenes the one-ray-per-lane kernels serve and that are small enough to be code (rm_rtc.h): expression forests, and --
    // as one single-leaf object per primitive -- primitive lists (up to 32) and sphere lists of fewer than `rtc_spheres` (16)
    // spheres, whose BVH has at most eight leaves (larger ones run in the v2 wave loop).
    ctx->rtc_src.clear();
    if (ctx->host.program) {
        ctx->rtc_src = rmrtc::scene_source(ctx->host.prog, ctx->host.obj_ranges, ctx->host.prog_tree, ctx->host.prog_roots, ctx->opt_prune != 0, ctx->host.bvh,
                                           ctx->host.bvh_prims, false);
    } else if (ctx->host.general ? ctx->host.prims.size() <= 32 : static_cast<int64_t>(ctx->host.spheres.size()) < ctx->opt_rtc_spheres) {
        std::vector<RmInstr> prog;
        std::vector<int32_t> ranges, roots;
        std::vector<rmh::ProgTreeNode> tree;
        if (rmh::leaf_objects(ctx->host, prog, ranges, tree, roots))
            ctx->rtc_src = rmrtc::scene_source(prog, ranges, tree, roots, false, ctx->host.bvh, ctx->host.bvh_prims, true);
    }
    ctx->cull_leaves = cull_leaf_table(ctx->host.bvh);
    if (!ctx->has_device) {
        free_device_scene(ctx);
        return RM_OK;
    }
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RM_HIP(ctx, hipDeviceSynchronize());  // nothing may still read the old tables
    free_device_scene(ctx);
    ctx->scene_gen++;  // the octree frame tables of the old scene are stale
    int rc;
#define RM_X(name, always) \
    if ((always || !ctx->host.name.empty()) && (rc = upload_vec(ctx, ctx->host.name, &ctx->dev.name))) return rc;
    RM_SCENE_ARRAYS(RM_X)
#undef RM_X
    ctx->dev.bvh_leaf_count = static_cast<int32_t>(ctx->cull_leaves.size());
    return upload_vec(ctx, ctx->cull_leaves, &ctx->dev.bvh_leaves);
}

int clamp_preset(int idx) { return idx < 0 ? 0 : (idx > rmh::kPresetCount - 1 ? rmh::kPresetCount - 1 : idx); }
int norm_accel(int a) { return (a == RM_ACCEL_OCTREE || a == RM_ACCEL_BVH) ? a : RM_ACCEL_NONE; }

int set_scene(rm_ctx *ctx, const SceneDesc &d, int accel, bool uploaded, int preset, const rmh::PairLoops *loops = nullptr) {
    std::string err;
    rmh::HostScene hs;
    rmh::set_length_mode(static_cast<int>(ctx->opt_length));
    bool ok = false;
    switch (d.kind) {
        case SceneDesc::kSpheres: ok = rmh::build_scene(hs, d.centers.data(), d.radii.data(), static_cast<int>(d.radii.size()), accel, err, loops); break;
        case SceneDesc::kPrims: ok = rmh::build_scene_general(hs, d.prims.data(), static_cast<int>(d.prims.size()), accel, err); break;
        case SceneDesc::kNodes:
            ok = rmh::build_scene_nodes(hs, d.nodes.data(), static_cast<int>(d.nodes.size()), d.roots.data(), static_cast<int>(d.roots.size()), accel, err);
            break;
    }
    if (!ok) {
        const bool unsupported = err.find("BVH leaf") != std::string::npos || (d.kind == SceneDesc::kNodes && err.find("RM_PROG_MAX") != std::string::npos);
        return fail(ctx, unsupported ? RM_E_UNSUPPORTED : RM_E_INVALID, err);
    }
    hs.preset = preset;
    ctx->host = std::move(hs);
    ctx->have_scene = true;
    ctx->scene_is_uploaded = uploaded;
    ctx->scene_preset = preset;
    return upload_scene(ctx);
}

// rm_scene_from_spheres / _prims / _nodes: the upload is remembered only once it has been built
int set_uploaded_scene(rm_ctx *ctx, SceneDesc &&d, int32_t accel) {
    const int rc = set_scene(ctx, d, norm_accel(accel), true, RM_SCENE_UPLOADED);
    if (rc) return rc;
    ctx->uploaded = std::move(d);
    ctx->have_uploaded = true;
    return RM_OK;
}

// a preset's objects as the builders take them: sphere presets as spheres, torus / box presets as general primitive records,
// operator / Mandelbulb presets as expression forests
bool preset_desc(int preset, SceneDesc &d) {
    d.kind = SceneDesc::kSpheres;
    if (rmh::preset_spheres(preset, d.centers, d.radii)) return true;
    d.kind = SceneDesc::kPrims;
    if (rmh::preset_prims(preset, d.prims)) return true;
    d.kind = SceneDesc::kNodes;
    return rmh::preset_nodes(preset, d.nodes, d.roots);
}

// ---- rm_scene_edit_spheres: the pair loops of the scene build on the device (rm_scene_build.hip) ---------------------------

struct DevMem {  // a device allocation that lives as long as the call that made it
    void *p = nullptr;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <typename T>
    hipError_t put(const T *src, size_t n, hipStream_t stream) {  // (src stays valid until the stream is synchronised)
        hipError_t e = alloc(n * sizeof(T));
        if (e == hipSuccess && n) e = hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, stream);
        return e;
    }
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

#define RM_TRY(call)                            \
    do {                                        \
        if ((call) != hipSuccess) return false; \
    } while (0)

// The candidate rule (rm_scene_host.cpp, build_point_query_grid) over `grids` on the device -> per cell the header
// (offset << 8) | count and the lists, byte for byte what the host loops produce.  `ids`: the table the grids' sphere ranges
// index (null: the scene's spheres themselves).  cap255: the rule of the two grids -- a cell of 255 or more candidates, or
// one that pass 1 marked (use_root: the exterior grid's cells inside the root box), keeps the header 255 and no list.
// `order`: the order in which the host appends the cells' lists (null: linear cell order).
// False, with hdr and list untouched, when the device failed or a list would reach 2^24 entries: that rule of the host's
// is sequential (it drops the cell that would pass the limit), so the host builds such a table.
template <typename E>
bool device_cand_lists(rm_ctx *ctx, const rmh::HostScene &s, const std::vector<int32_t> *ids, const std::vector<RmCandGrid> &grids,
                       int cells_per_grid, double u0, bool use_root, bool cap255, const std::vector<uint32_t> *order,
                       std::vector<uint32_t> &hdr, std::vector<E> &list) {
    const size_t n = s.spheres.size(), n_cells = grids.size() * static_cast<size_t>(cells_per_grid);
    if (!n || !n_cells || n != s.radii.size() || n > 0x7FFFFFFFu || (order && order->size() != n_cells)) return false;
    RM_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<double> sp(4 * n);
    for (size_t i = 0; i < n; ++i) {
        sp[4 * i] = s.spheres[i].cx;
        sp[4 * i + 1] = s.spheres[i].cy;
        sp[4 * i + 2] = s.spheres[i].cz;
        sp[4 * i + 3] = s.radii[i];
    }
    DevMem d_sp, d_ids, d_grids, d_counts, d_u, d_off, d_list;
    RM_TRY(d_sp.put(sp.data(), sp.size(), st));
    if (ids) RM_TRY(d_ids.put(ids->data(), ids->size(), st));
    RM_TRY(d_grids.put(grids.data(), grids.size(), st));
    RM_TRY(d_counts.alloc(n_cells * sizeof(uint32_t)));
    RM_TRY(d_u.alloc(n_cells * sizeof(double)));
    RmCandArgs a = {};
    a.grids = d_grids.as<RmCandGrid>();
    a.spheres = d_sp.as<double>();
    a.ids = ids ? d_ids.as<int32_t>() : nullptr;
    a.counts = d_counts.as<uint32_t>();
    a.u = d_u.as<double>();
    a.n_cells = static_cast<long long>(n_cells);
    a.u0 = u0;
    for (int k = 0; k < 3; ++k) {
        a.root_lo[k] = s.root_min[k];
        a.root_hi[k] = s.root_max[k];
    }
    a.n_grids = static_cast<int32_t>(grids.size());
    a.cells_per_grid = cells_per_grid;
    a.n_spheres = static_cast<int32_t>(n);
    a.n_ids = ids ? static_cast<int32_t>(ids->size()) : 0;
    a.use_root = use_root ? 1 : 0;
    RM_TRY(rm_launch_cand_count(a, st));
    std::vector<uint32_t> counts(n_cells);
    RM_TRY(hipMemcpyAsync(counts.data(), d_counts.p, n_cells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RM_TRY(hipStreamSynchronize(st));
    std::vector<uint32_t> offs(n_cells), h(n_cells);
    size_t total = 0;
    for (size_t i = 0; i < n_cells; ++i) {
        const size_t c = order ? (*order)[i] : i;
        if (c >= n_cells) return false;
        const uint32_t cnt = counts[c];
        if (cnt == RM_CAND_NO_LIST || cnt >= (cap255 ? 255u : 256u)) {
            if (!cap255) return false;
            offs[c] = RM_CAND_NO_LIST;
            h[c] = 255;
            continue;
        }
        if (total + cnt >= (1u << 24)) return false;
        offs[c] = static_cast<uint32_t>(total);
        h[c] = static_cast<uint32_t>(total << 8) | cnt;
        total += cnt;
    }
    std::vector<E> out(total);
    if (total) {
        RM_TRY(d_off.put(offs.data(), offs.size(), st));
        RM_TRY(d_list.alloc(total * sizeof(E)));
        a.offsets = d_off.as<uint32_t>();
        a.list_len = total;
        RM_TRY(rm_launch_cand_fill(a, d_list.p, static_cast<int>(sizeof(E)), st));
        RM_TRY(hipMemcpyAsync(out.data(), d_list.p, total * sizeof(E), hipMemcpyDeviceToHost, st));
        RM_TRY(hipStreamSynchronize(st));
    }
    hdr.swap(h);
    list.swap(out);
    return true;
}

// rmh::PairLoops served by the device
rmh::PairLoops device_pair_loops(rm_ctx *ctx) {
    rmh::PairLoops L;
    L.nn_grid = [ctx](rmh::HostScene &s) {
        RmCandGrid g = {};
        int cells = 1;
        for (int k = 0; k < 3; ++k) {
            g.org[k] = double(s.pq_origin[k]);
            g.w[k] = s.nn_inv[k] > 0 ? 1.0 / double(s.nn_inv[k]) : 0.0;
            g.dim[k] = s.nn_dim[k];
            cells *= s.nn_dim[k];
        }
        g.n = static_cast<int32_t>(s.spheres.size());
        std::vector<uint32_t> hdr;
        std::vector<uint16_t> list;
        if (!device_cand_lists<uint16_t>(ctx, s, nullptr, {g}, cells, 10.0, false, true, nullptr, hdr, list)) return false;
        s.nn_cells.swap(hdr);
        s.nn_list.swap(list);
        return true;
    };
    L.ext_grid = [ctx](rmh::HostScene &s) {
        RmCandGrid g = {};
        const int dim = s.ext_dim[0];
        if (dim <= 0 || dim % 4 || s.ext_dim[1] != dim || s.ext_dim[2] != dim) return false;
        for (int k = 0; k < 3; ++k) {
            g.org[k] = double(s.ext_origin[k]);
            g.w[k] = 1.0 / double(s.ext_inv[k]);
            g.dim[k] = dim;
        }
        g.n = static_cast<int32_t>(s.spheres.size());
        // the host appends the lists block by block (4^3 cells, build_exterior_grid): the offsets follow that order
        std::vector<uint32_t> order;
        order.reserve(static_cast<size_t>(dim) * dim * dim);
        for (int bz = 0; bz < dim; bz += 4)
            for (int by = 0; by < dim; by += 4)
                for (int bx = 0; bx < dim; bx += 4)
                    for (int z = bz; z < bz + 4; ++z)
                        for (int y = by; y < by + 4; ++y)
                            for (int x = bx; x < bx + 4; ++x) order.push_back(static_cast<uint32_t>((z * dim + y) * dim + x));
        std::vector<uint32_t> hdr;
        std::vector<uint16_t> list;
        if (!device_cand_lists<uint16_t>(ctx, s, nullptr, {g}, dim * dim * dim, 10.0, true, true, &order, hdr, list)) return false;
        s.ext_cells.swap(hdr);
        s.ext_list.swap(list);
        return true;
    };
    L.oct_sub = [ctx](rmh::HostScene &s, const std::vector<int32_t> &leaves) {
        const int kSub = RM_OCT_SUB * RM_OCT_SUB * RM_OCT_SUB;
        std::vector<RmCandGrid> grids(leaves.size());
        for (size_t i = 0; i < leaves.size(); ++i) {
            if (leaves[i] < 0 || static_cast<size_t>(leaves[i]) >= s.oct.size()) return false;
            const RmOctNode &nd = s.oct[leaves[i]];
            RmCandGrid &g = grids[i];
            g = RmCandGrid{};
            for (int k = 0; k < 3; ++k) {
                g.org[k] = double(nd.lo[k]);
                g.w[k] = (double(nd.hi[k]) - double(nd.lo[k])) / double(RM_OCT_SUB);
                g.dim[k] = RM_OCT_SUB;
            }
            g.first = nd.prim_first;
            g.n = nd.prim_count;
        }
        std::vector<uint32_t> hdr;
        std::vector<uint8_t> list;
        if (!device_cand_lists<uint8_t>(ctx, s, &s.oct_prims, grids, kSub, std::numeric_limits<double>::infinity(), false, false, nullptr,
                                        hdr, list))
            return false;
        for (size_t i = 0; i < leaves.size(); ++i)  // the host stops at the first leaf that could pass 2^24 entries
            if ((hdr[i * kSub] >> 8) + static_cast<size_t>(kSub) * static_cast<size_t>(s.oct[leaves[i]].prim_count) >= (1u << 24)) return false;
        s.oct_sub_hdr.swap(hdr);
        s.oct_sub_list.swap(list);
        return true;
    };
    L.empty_dist = [ctx](const rmh::HostScene &s, const std::vector<int32_t> &nodes, std::vector<double> &out) {
        const size_t n_prims = s.prim_lo.size() / 3;
        if (nodes.empty() || nodes.size() > 0x7FFFFFFFu || n_prims > 0x7FFFFFFFu || s.prim_hi.size() != s.prim_lo.size()) return false;
        std::vector<float> boxes(6 * nodes.size());
        for (size_t i = 0; i < nodes.size(); ++i) {
            if (nodes[i] < 0 || static_cast<size_t>(nodes[i]) >= s.oct.size()) return false;
            std::memcpy(&boxes[6 * i], s.oct[nodes[i]].lo, 3 * sizeof(float));
            std::memcpy(&boxes[6 * i + 3], s.oct[nodes[i]].hi, 3 * sizeof(float));
        }
        RM_TRY(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        DevMem d_boxes, d_lo, d_hi, d_out;
        RM_TRY(d_boxes.put(boxes.data(), boxes.size(), st));
        RM_TRY(d_lo.put(s.prim_lo.data(), s.prim_lo.size(), st));
        RM_TRY(d_hi.put(s.prim_hi.data(), s.prim_hi.size(), st));
        RM_TRY(d_out.alloc(nodes.size() * sizeof(double)));
        RmEmptyDistArgs a = {};
        a.boxes = d_boxes.as<float>();
        a.prim_lo = d_lo.as<float>();
        a.prim_hi = d_hi.as<float>();
        a.out = d_out.as<double>();
        a.n_nodes = static_cast<int32_t>(nodes.size());
        a.n_prims = static_cast<int32_t>(n_prims);
        RM_TRY(rm_launch_empty_dist(a, st));
        std::vector<double> d(nodes.size());
        RM_TRY(hipMemcpyAsync(d.data(), d_out.p, d.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        RM_TRY(hipStreamSynchronize(st));
        out.swap(d);
        return true;
    };
    return L;
}
#undef RM_TRY

int scene_n_prims(const rm_ctx *ctx) {
    if (ctx->host.program) return static_cast<int>(ctx->host.obj_ranges.size() / 2);
    return static_cast<int>(ctx->host.general ? ctx->host.prims.size() : ctx->host.spheres.size());
}

// The active scene as every kernel that evaluates it reads it (render, ray query and rm_scene_distance alike): which primitive
// representation (RmRenderParams::general), the counts, the primitive tables and the two trees, and the exterior
// candidate grid (option `ext`).  What only the render kernels read -- the leaf grid, its candidate lists, octree records -- is
// fill_params' business and stays null / zero elsewhere.
void fill_scene_view(const rm_ctx *ctx, RmRenderParams &p) {
    p.n_prims = scene_n_prims(ctx);
    p.general = ctx->host.general ? 1 : 0;
    if (ctx->host.program) {
        p.general = 2;
        for (const RmInstr &ins : ctx->host.prog)
            if (ins.op == 3) p.general = 3;  // Mandelbulb leaf: the instantiation that carries the fdlibm code
    }
    p.prims = ctx->dev.prims;
    p.prog = ctx->dev.prog;
    p.obj_ranges = ctx->dev.obj_ranges;
    p.prog_slots = ctx->host.prog_slots;
    p.prog_vals = ctx->host.prog_vals;
    p.accel = ctx->host.accel;
    p.bvh_nodes = static_cast<int32_t>(ctx->host.bvh.size());
    p.oct_nodes = static_cast<int32_t>(ctx->host.oct.size());
    p.spheres = ctx->dev.spheres;
    p.radii = ctx->dev.radii;
    p.bvh = ctx->dev.bvh;
    p.bvh_prims = ctx->dev.bvh_prims;
    p.oct = ctx->dev.oct;
    p.oct_prims = ctx->dev.oct_prims;
    p.oct_lut = ctx->opt_lut ? ctx->dev.oct_lut : nullptr;
    // the exterior candidate grid (points outside the BVH root box): read by the v2 wave loop and rm_debug_wave_distance only -- the
    // one-ray-per-lane kernels (kernel = 1, rm_scene_distance, ray queries) ignore it and evaluate all N there
    p.ext_cells = ctx->dev.ext_cells;
    p.ext_list = ctx->dev.ext_list;
    for (int k = 0; k < 3; ++k) {
        p.ext_dim[k] = ctx->host.ext_dim[k];
        p.ext_origin[k] = ctx->host.ext_origin[k];
        p.ext_inv[k] = ctx->host.ext_inv[k];
    }
    p.use_ext = (ctx->opt_ext && ctx->host.accel == RM_ACCEL_BVH && !ctx->host.ext_cells.empty() && ctx->host.ext_dim[0] > 0) ? 1 : 0;
}

// The parameter block of a query without a ray (rm_scene_distance, and the field, point, sharp-vertex, block and tile launches):
// the active scene at `time` -- ctx->time is not touched --, the ahead-of-time kernels (rm_scene_distance alone names its
// specialised kernel afterwards).
void fill_scene_query(const rm_ctx *ctx, double time, RmRenderParams &p) {
    std::memset(&p, 0, sizeof p);
    fill_scene_view(ctx, p);
    p.time = time;
    p.filter = static_cast<int32_t>(ctx->opt_filter);
    p.tile_w = 8;
    p.rtc_function = nullptr;
}

// Option `exact`: what the next exact query of the active scene walks (rmh::exact_tree_mode), decided -- and, for an own tree,
// built on the host and copied up, synchronously -- once per scene; free_device_scene drops it with the scene.  A tree that
// cannot be built or uploaded leaves mode 0 (every object), which answers the same values.
int ensure_exact_tree(rm_ctx *ctx) {
    if (ctx->exact_ready) return RM_OK;
    int mode = rmh::exact_tree_mode(ctx->host);
    if (mode == 2 && !rmh::build_exact_tree(ctx->host, ctx->exact_tree)) mode = 0;
    if (mode == 2 && ctx->has_device) {
        RM_HIP(ctx, hipSetDevice(ctx->device));
        int rc;
        if ((rc = upload_vec(ctx, ctx->exact_tree.nodes, &ctx->d_exact_nodes))) return rc;
        if ((rc = upload_vec(ctx, ctx->exact_tree.ids, &ctx->d_exact_ids))) return rc;
    }
    ctx->exact_mode = mode;
    ctx->exact_ready = true;
    return RM_OK;
}

// The parameter block of a point, field or tile launch under option `exact`: the exact instantiation and the tree it walks
// (RM_ACCEL_EXACT, rm_kernels.h).  Without the option the block stays as it is.  use_exact: the same whatever the option says
// (rm_scene_tiles_update_device is defined for the exact field only).
int use_exact(rm_ctx *ctx, RmRenderParams &p) {
    const int rc = ensure_exact_tree(ctx);
    if (rc) return rc;
    p.accel = RM_ACCEL_EXACT;
    if (ctx->exact_mode == 2) {
        p.bvh = ctx->d_exact_nodes;
        p.bvh_prims = ctx->d_exact_ids;
        p.bvh_nodes = static_cast<int32_t>(ctx->exact_tree.nodes.size());
    } else if (ctx->exact_mode == 0) {
        p.bvh_nodes = 0;
    }
    p.use_ext = 0;
    return RM_OK;
}
int apply_exact(rm_ctx *ctx, RmRenderParams &p) { return ctx->opt_exact ? use_exact(ctx, p) : static_cast<int>(RM_OK); }


// makes the scene named by the job the active one (raymarchWorker.ts:37-38)
int ensure_scene(rm_ctx *ctx, int32_t preset_index, int32_t accel_in) {
    const int accel = norm_accel(accel_in);
    if (preset_index == RM_SCENE_UPLOADED) {
        if (!ctx->have_uploaded) return fail(ctx, RM_E_NO_SCENE, "no scene uploaded with rm_scene_from_spheres");
        if (ctx->have_scene && ctx->scene_is_uploaded && ctx->host.accel == accel) return RM_OK;
        return set_scene(ctx, ctx->uploaded, accel, true, RM_SCENE_UPLOADED);
    }
    const int preset = clamp_preset(preset_index);
    if (ctx->have_scene && !ctx->scene_is_uploaded && ctx->scene_preset == preset && ctx->host.accel == accel)
        return RM_OK;
    SceneDesc d;
    if (preset_desc(preset, d)) return set_scene(ctx, d, accel, false, preset);
    return fail(ctx, RM_E_UNSUPPORTED, "scene preset " + std::to_string(preset) + " is not on the native path");
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Staging of one call's host buffers through the context's scratch buffer, on the context's stream.  region() lays the
// regions out in the order they are named, each 256-byte aligned, and returns their offsets; reserve() grows the scratch
// once to hold them all (it never shrinks, and the device is synchronised before an old buffer is freed) and asks for 256
// bytes at least, so at() is a device pointer even when every region is empty.  in / zero / out are enqueued.
// An asynchronous entry reserves for the caller's stream and calls keep() behind its launches (scratch_call): whoever reserves
// next, on whatever stream, waits on the device for them, so two users of the scratch never overlap.
struct Staging {
    rm_ctx *ctx;
    size_t total = 0;
    size_t region(size_t bytes) {
        const size_t offset = total;
        total += align_up(bytes, 256);
        return offset;
    }
    int reserve() const { return reserve_for(ctx->stream); }
    int reserve_for(hipStream_t user) const {
        if (ctx->scratch_busy) RM_HIP(ctx, hipStreamWaitEvent(user, ctx->scratch_busy, 0));
        const size_t bytes = total ? total : 256;
        if (bytes <= ctx->scratch_bytes) return RM_OK;
        if (ctx->scratch) {
            RM_HIP(ctx, hipDeviceSynchronize());
            (void)hipFree(ctx->scratch);
            ctx->scratch = nullptr;
            ctx->scratch_bytes = 0;
        }
        RM_HIP(ctx, hipMalloc(&ctx->scratch, bytes));
        ctx->scratch_bytes = bytes;
        return RM_OK;
    }
    template <typename T>
    T *at(size_t offset) const { return reinterpret_cast<T *>(static_cast<char *>(ctx->scratch) + offset); }
    hipError_t in(size_t offset, const void *host, size_t bytes) const { return hipMemcpyAsync(at<char>(offset), host, bytes, hipMemcpyHostToDevice, ctx->stream); }
    hipError_t zero(size_t offset, size_t bytes) const { return hipMemsetAsync(at<char>(offset), 0, bytes, ctx->stream); }
    hipError_t out(void *host, size_t offset, size_t bytes) const { return hipMemcpyAsync(host, at<char>(offset), bytes, hipMemcpyDeviceToHost, ctx->stream); }
    hipError_t sync() const { return hipStreamSynchronize(ctx->stream); }
    hipError_t keep(hipStream_t user) const {
        if (!ctx->scratch_busy) {
            const hipError_t e = hipEventCreateWithFlags(&ctx->scratch_busy, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(ctx->scratch_busy, user);
    }
};

// An asynchronous entry that needs room in the scratch buffer, behind its checks; `bytes`: its regions in order (four at most).
// With `work` they are reserved for the caller's stream, launch(st, o) -- o[i] the offset of region i -- enqueues the kernels and
// returns an RM_* code, and keep() follows whatever that code is: what a launch that failed half way did enqueue reads the
// scratch too.  Without work there is no launch: info_bytes at d_info (null: none) are zeroed on the stream.
template <typename Launch>
int scratch_call(rm_ctx *ctx, hipStream_t stream, bool work, void *d_info, size_t info_bytes, std::initializer_list<size_t> bytes, Launch launch) {
    RM_HIP(ctx, hipSetDevice(ctx->device));
    if (!work) {
        if (d_info) RM_HIP(ctx, hipMemsetAsync(d_info, 0, info_bytes, stream));
        return RM_OK;
    }
    Staging st{ctx};
    size_t o[4] = {0, 0, 0, 0}, *next = o;
    for (const size_t b : bytes) *next++ = st.region(b);
    if (const int rc = st.reserve_for(stream)) return rc;
    const int rc = launch(st, o);
    const hipError_t kept = st.keep(stream);
    if (rc) return rc;
    RM_HIP(ctx, kept);
    return RM_OK;
}

// One buffer of a call that has a device form and a host form (staged_call): the caller's pointer -- device or host by the form;
// null: not asked for, no staging bytes and a null kernel pointer --, its bytes per element, where the kernel's argument block
// takes its pointer, and which way the host form copies it.  over >= 0: the column has no region of its own, the kernel writes
// it over the staged column of that index, which is always asked for (rm_scene_points: the positions over the points; the
// kernel reads an element before it writes it).
struct Column {
    const void *ptr;
    size_t bytes;
    void *slot;      // the pointer member of the argument block that this column feeds
    bool in, out;    // host form: the caller's content goes in ahead of the launch / comes back behind it
    int over = -1;
};
constexpr int kMaxColumns = 10;
// What a host form takes through the scratch at a time unless its records are large: 4 M elements -- 208 MB with a march's
// columns, 224 MB a pick's, 272 MB a light's, 288 MB of walk summaries, 192 MB of a point query's, 64 MB of a field's.
constexpr int64_t kHostChunk = int64_t(1) << 22;

// Both forms of a query or a frame operation over n > 0 elements (rays, points, lattice points, vertices, pixels, whole frames),
// behind its checks.  launch(first, m, stream) enqueues the kernel for elements
// [first, first + m) with every column's pointer fed and indexed from `first`.  host false: the columns are the caller's device
// buffers, one launch of all n on `stream`.  host true: through the scratch buffer on the context's stream in chunks of at most
// `limit` elements, whole rows of `row` (a row at least; n is a multiple of row), synchronous; only the columns asked for are
// staged and copied; limit = n makes it one trip and one launch.  Nothing here depends on the caller.
template <typename Launch>
int staged_call(rm_ctx *ctx, bool host, hipStream_t stream, int64_t n, int64_t row, int64_t limit, const Column *cols, int n_cols, Launch launch) {
    const auto feed = [](const Column &col, const void *ptr) { std::memcpy(col.slot, &ptr, sizeof ptr); };
    if (!host) {
        for (int j = 0; j < n_cols; ++j) feed(cols[j], cols[j].ptr);
        RM_HIP(ctx, launch(int64_t(0), n, stream));
        return RM_OK;
    }
    const int64_t chunk = std::min(n, std::max<int64_t>(1, limit / row) * row);
    Staging st{ctx};
    size_t o_col[kMaxColumns];
    for (int j = 0; j < n_cols; ++j)
        o_col[j] = cols[j].over >= 0 ? o_col[cols[j].over] : st.region(cols[j].ptr ? cols[j].bytes * static_cast<size_t>(chunk) : 0);
    if (const int rc = st.reserve()) return rc;
    for (int j = 0; j < n_cols; ++j) feed(cols[j], cols[j].ptr ? st.at<char>(o_col[j]) : nullptr);
    for (int64_t s = 0; s < n; s += chunk) {
        const int64_t m = n - s < chunk ? n - s : chunk;
        const size_t k = static_cast<size_t>(m), at = static_cast<size_t>(s);
        for (int j = 0; j < n_cols; ++j) {
            const Column &col = cols[j];
            if (col.ptr && col.in) RM_HIP(ctx, st.in(o_col[j], static_cast<const char *>(col.ptr) + at * col.bytes, col.bytes * k));
        }
        RM_HIP(ctx, launch(s, m, ctx->stream));
        for (int j = 0; j < n_cols; ++j) {
            const Column &col = cols[j];
            if (col.ptr && col.out) RM_HIP(ctx, st.out(static_cast<char *>(const_cast<void *>(col.ptr)) + at * col.bytes, o_col[j], col.bytes * k));
        }
        RM_HIP(ctx, st.sync());  // the next chunk reuses the scratch
    }
    return RM_OK;
}

// Why a launch of the active scene with this camera and frame would not cull by leaf rectangles (option `rect_cull`): 0 it would,
// 1 the options (`rect_cull`, `cull`) or the scene's kind (no BVH, or a tree the cull does not serve), 2 more leaves than
// a launch keeps rectangles for (the bundle cull itself stops there), 3 the camera (rm_rect_cull_camera_ok) or a frame beyond 65 536 pixels a side.  Whether the
// launch runs the wave loop at all is fill_params' to say.
int rect_cull_refusal(const rm_ctx *ctx, const float rot[9], const float origin[3], int32_t width, int32_t height) {
    if (!ctx->opt_rect_cull || !ctx->opt_cull || ctx->host.accel != RM_ACCEL_BVH) return 1;
    if (ctx->cull_leaves.size() > RM_RECT_CULL_MAX_LEAVES || (ctx->cull_leaves.empty() && ctx->host.bvh_leaves > RM_RECT_CULL_MAX_LEAVES)) return 2;
    if (ctx->cull_leaves.empty()) return 1;
    if (!rm_rect_cull_camera_ok(rot, origin) || width < 1 || height < 1 || width > 65536 || height > 65536) return 3;
    return 0;
}

int fill_params(rm_ctx *ctx, const rm_job *job, RmRenderParams &p) {
    if (!job) return fail(ctx, RM_E_INVALID, "null job");
    if (job->height <= 0 || job->width < 0) return fail(ctx, RM_E_INVALID, "width must be >= 0 and height > 0");
    if (!std::isfinite(job->camera_pitch) || !std::isfinite(job->camera_yaw))
        return fail(ctx, RM_E_INVALID, "non-finite camera angle");
    if (job->algorithm < RM_ALG_SPHERE_TRACER || job->algorithm > RM_ALG_ADAPTIVE_STEP_V3)
        return fail(ctx, RM_E_INVALID, "unknown algorithm enum (use rm_algorithm_from_string)");
    int rc = ensure_scene(ctx, job->scene_preset_index, job->acceleration_structure);
    if (rc) return rc;
    std::memset(&p, 0, sizeof p);
    p.width = job->width;
    p.height = job->height;
    p.y_start = job->y_start;
    p.y_end = job->y_end;
    p.algorithm = job->algorithm;
    // NaN stands for JS `undefined`: the constructors' defaults (adaptiveStepV2.ts:13, fixedStep.ts:13)
    p.overshoot = std::isnan(job->overshoot_factor) ? 1.2 : job->overshoot_factor;
    p.step_size = std::isnan(job->step_size) ? 0.1 : job->step_size;
    p.local_rows = job->y_end > job->y_start ? job->y_end - job->y_start : 0;
    p.stripe_rows = 0;
    p.n_parts = 1;
    p.part = 0;
    rmh::camera_from_angles(job->camera_pitch, job->camera_yaw, p.rot, p.origin);
    std::memcpy(p.light, ctx->light, sizeof p.light);
    for (int k = 0; k < 9; ++k) p.rot_d[k] = p.rot[k];
    for (int k = 0; k < 3; ++k) {
        p.origin_d[k] = p.origin[k];
        p.light_d[k] = p.light[k];
    }
    fill_scene_view(ctx, p);
    if (!std::isfinite(job->time)) return fail(ctx, RM_E_INVALID, "non-finite time");
    ctx->time = job->time;  // raymarcher.ts:58-59 scene.updateTime(time)
    p.time = job->time;
    p.tile_w = static_cast<int32_t>(ctx->opt_tile_w);
    p.nodes_in_lds = static_cast<int32_t>(ctx->opt_lds);
    p.filter = static_cast<int32_t>(ctx->opt_filter);
    p.variant = static_cast<int32_t>(ctx->opt_kernel);
    // auto: the octree runs in the one-ray-per-lane kernels; so do the smallest scenes.  (Until round 2 the 9-sphere grid of C2
    // was faster there too; since the in-round march steps of round 3 the uniform wave loop wins it: 0.308 against 0.331 ms
    // alone, 9 680 against 8 920 frames/s in flight.)
    if (p.variant == 0)
        p.variant = (ctx->host.accel == RM_ACCEL_OCTREE || ctx->host.spheres.size() < 8 ||
                     (ctx->opt_specialise && !ctx->rtc_src.empty() && rmrtc::available(nullptr) &&
                      static_cast<int64_t>(ctx->host.spheres.size()) < ctx->opt_rtc_spheres))
                        ? 1
                        : 2;
    if (p.algorithm != RM_ALG_SPHERE_TRACER) p.variant = 1;  // the other marchers live in the v1 kernel
    if (ctx->host.general) p.variant = 1;                    // so do boxes, tori and rotated primitives
    // v1: square 8 x 8 wave tiles keep a wave's rays in the same leaves / intervals (N3-mixed 2.31 -> 2.07 ms together with
    // one-wave workgroups, option `v1_block`)
    if (p.variant == 1 && !ctx->tile_w_set) p.tile_w = 8;
    p.list_cap = static_cast<int32_t>(ctx->opt_list_cap);
    p.coop = static_cast<int32_t>(ctx->opt_coop);
    p.bvh_prim_count = static_cast<int32_t>(ctx->host.bvh_prims.size());
    p.oct_prim_count = static_cast<int32_t>(ctx->host.oct_prims.size());
    p.blocks_per_cu = static_cast<int32_t>(ctx->opt_blocks_per_cu);
    p.launch_per_cu = launch_fill(p.blocks_per_cu, ctx->hw_queues, ctx->opt_min_fill != 0);
    p.overlap_per_cu = overlap_fill(p.blocks_per_cu, ctx->hw_queues, ctx->opt_min_fill != 0, ctx->opt_overlap_fill != 0);
    p.num_cus = ctx->num_cus;
    p.refill_threshold = static_cast<int32_t>(ctx->opt_refill);
    p.hw_xcd = static_cast<int32_t>(ctx->opt_hw_xcd);
    p.item_px = static_cast<int32_t>(ctx->opt_item_px);
    p.stamps = ctx->d_stamps;
    for (int k = 0; k < 3; ++k) {
        p.pq_dim[k] = ctx->host.pq_dim[k];
        p.pq_origin[k] = ctx->host.pq_origin[k];
        p.pq_inv[k] = ctx->host.pq_inv[k];
        // cell size, rounded down a little: it scales a distance that must not be overstated
        p.pq_cell[k] = ctx->host.pq_inv[k] > 0.f ? static_cast<float>((1.0 / static_cast<double>(ctx->host.pq_inv[k])) * 0.9999) : 0.f;
    }
    p.pq_cell_count = static_cast<int32_t>(ctx->host.pq_cells.size());
    p.pq_list_count = static_cast<int32_t>(ctx->host.pq_list.size());
    p.use_grid = (ctx->opt_grid && !ctx->host.pq_cells.empty()) ? 1 : 0;
    p.pq_cells = ctx->dev.pq_cells;
    p.pq_list = ctx->dev.pq_list;
    p.bvh_leaves = ctx->dev.bvh_leaves;
    p.bvh_leaf_count = (ctx->opt_cull && ctx->host.accel == RM_ACCEL_BVH) ? ctx->dev.bvh_leaf_count : 0;
    p.rect_cull = rect_cull_refusal(ctx, p.rot, p.origin, p.width, p.height) == 0 ? 1 : 0;  // (the launch's table: launch_render)
    p.nn_cells = ctx->dev.nn_cells;
    p.nn_list = ctx->dev.nn_list;
    p.nn_cell_count = static_cast<int32_t>(ctx->host.nn_cells.size());
    p.nn_list_count = static_cast<int32_t>(ctx->host.nn_list.size());
    const bool nn_on = ctx->opt_nn == 1 || (ctx->opt_nn == 2 && ctx->host.spheres.size() <= 512);
    p.use_nn = (p.use_grid && nn_on && !ctx->host.nn_cells.empty()) ? 1 : 0;
    p.leaf_order = ctx->host.leaf_order ? 1 : 0;
    p.rel_boxes = static_cast<int32_t>(ctx->opt_rel);
    p.n0_batch = static_cast<int32_t>(ctx->opt_n0_batch);
    p.v1_lists = static_cast<int32_t>(ctx->opt_v1_lists);
    p.v1_block = static_cast<int32_t>(ctx->opt_v1_block);
    p.oct_lean = static_cast<int32_t>(ctx->opt_oct_lean);  // the camera is finite (fill_params), so every march point is
    p.v1_list_offset = -1;
    p.prim_filter = (ctx->opt_filter && ctx->host.general && !ctx->host.program && ctx->host.prim_filter_ok &&
                     ctx->host.spheres.size() == ctx->host.prims.size()) ? 1 : 0;
    p.lds_budget_kb = static_cast<int32_t>(ctx->opt_lds_kb);
    p.lds_fill = static_cast<int32_t>(ctx->opt_lds_fill);
    p.item_wide = static_cast<int32_t>(ctx->opt_item_wide);
    p.multi_step = static_cast<int32_t>(ctx->opt_multi_step);
    // the step-box table of section M: asked for here, granted by the launcher (rm_v2_plan).  A context with a device reads it
    // there; one without plans as if it had.
    p.step_tab = ctx->dev.step_tab;
    p.sb_bins = ctx->host.sb_bins;
    p.sb_stride = ctx->host.sb_stride;
    for (int k = 0; k < 3; ++k) {
        p.sb_origin[k] = ctx->host.sb_origin[k];
        p.sb_inv[k] = ctx->host.sb_inv[k];
    }
    p.step_box = (ctx->opt_step_box && ctx->opt_multi_step && ctx->host.accel == RM_ACCEL_BVH && !ctx->host.step_tab.empty() &&
                  (ctx->dev.step_tab || !ctx->has_device)) ? 1 : 0;
    // ... and the cell table of sections B, M and N: it goes with the step-box table (its records are indices into it)
    p.cell_tab = ctx->dev.cell_tab;
    p.ct_rec_off = ctx->host.ct_rec_off;
    p.ct_list_off = ctx->host.ct_list_off;
    p.ct_words = static_cast<int32_t>(ctx->host.cell_tab.size());
    for (int k = 0; k < 3; ++k) p.ct_dim[k] = ctx->host.ct_dim[k];
    p.cell_on = (ctx->opt_cell_tab && p.step_box && !ctx->host.cell_tab.empty() && (ctx->dev.cell_tab || !ctx->has_device)) ? 1 : 0;
    p.runner_up = (ctx->opt_runner_up && p.cell_on) ? 1 : 0;  // (and a one-radius scene: the launcher's to see, rm_v2_plan)
    p.uniform_radius = 0;
    if (ctx->opt_uniform && !ctx->host.general && ctx->host.spheres.size() >= 2 &&
        ctx->host.spheres.size() <= 256) {  // one radius, bit for bit; at most 256 spheres: the scan keys carry the id in eight bits
        const auto &sp = ctx->host.spheres;
        const auto &rd = ctx->host.radii;
        bool same = rd.size() == sp.size();
        for (size_t k = 1; same && k < sp.size(); ++k)
            same = std::memcmp(&sp[k].rf, &sp[0].rf, sizeof(float)) == 0 && std::memcmp(&rd[k], &rd[0], sizeof(double)) == 0;
        p.uniform_radius = same ? 1 : 0;
    }
    for (int k = 0; k < 3; ++k) {
        p.nn_dim[k] = ctx->host.nn_dim[k];
        p.nn_inv[k] = ctx->host.nn_inv[k];
    }
    p.oct_recs = ctx->opt_recs ? ctx->dev.oct_recs : nullptr;
    p.oct_sub_hdr = (ctx->opt_sub && ctx->opt_recs) ? ctx->dev.oct_sub_hdr : nullptr;
    p.oct_sub_list = ctx->dev.oct_sub_list;
    return RM_OK;
}

// rm_selftest_fastdiv and rm_selftest_recip: a kernel counts mismatches into one zeroed word of the scratch, read back alone
template <typename Launch>
int read_mismatches(rm_ctx *ctx, Launch launch, uint64_t *mismatches) {
    RM_HIP(ctx, hipSetDevice(ctx->device));
    Staging st{ctx};
    const size_t o = st.region(sizeof(unsigned long long));
    const int rc = st.reserve();
    if (rc) return rc;
    RM_HIP(ctx, st.zero(o, sizeof(unsigned long long)));
    RM_HIP(ctx, launch(st.at<unsigned long long>(o)));
    unsigned long long h = 0;
    RM_HIP(ctx, st.out(&h, o, sizeof h));
    RM_HIP(ctx, st.sync());
    *mismatches = h;
    return RM_OK;
}

int norm_shader(int s) { return (s >= RM_SHADE_NORMAL && s <= RM_SHADE_ITERATION_HEATMAP) ? s : RM_SHADE_NORMAL; }

// The parameter block of a ray query: what a one-ray-per-lane render launch of the ACTIVE scene reads (fill_params with a job
// that names that scene, so every knob applies as it does there), the query's marcher, step rules and time.  A query is pure:
// unlike a render it leaves the scene's time (rm_scene_set_time, what rm_scene_distance uses) as it was.  No run-time
// specialised kernel: cast_kernel and pick_kernel are ahead-of-time only.
int fill_query_params(rm_ctx *ctx, const rm_ray_query *q, RmRenderParams &p) {
    const double scene_time = ctx->time;
    rm_job job;
    std::memset(&job, 0, sizeof job);
    job.width = 1;
    job.height = 1;
    job.y_end = 1;
    job.time = q->time;
    const bool known = q->algorithm >= RM_ALG_SPHERE_TRACER && q->algorithm <= RM_ALG_ADAPTIVE_STEP_V3;
    job.algorithm = known ? q->algorithm : RM_ALG_SPHERE_TRACER;  // raymarchWorker.ts:49-68: the default branch
    job.scene_preset_index = ctx->scene_is_uploaded ? RM_SCENE_UPLOADED : ctx->scene_preset;
    job.acceleration_structure = ctx->host.accel;
    job.overshoot_factor = q->overshoot_factor;
    job.step_size = q->step_size;
    const int rc = fill_params(ctx, &job, p);
    ctx->time = scene_time;  // (fill_params stores the job's time there: raymarcher.ts:58-59 belongs to runRaymarcher only)
    p.rtc_function = nullptr;
    return rc;
}

// the checks every ray query makes
int check_query(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *origins, const void *dirs) {
    if (!q) return fail(ctx, RM_E_INVALID, "null query");
    if (n < 0 || n > std::numeric_limits<int32_t>::max()) return fail(ctx, RM_E_INVALID, "ray count out of range");
    if (n > 0 && (!origins || !dirs)) return fail(ctx, RM_E_INVALID, "null ray buffer");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU ray path");
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    return RM_OK;
}

// One call of a ray query as data.  ray_call owns it and names the rays as its first two columns; the family's describer fills
// the rest in place (so a column can point at the member it feeds): `args`, the kernel's argument block, with the non-pointer
// fields, `launch` the family's launcher by option `length`, `chunk` the most rays the host form takes through the scratch
// buffer at a time, and a column per buffer beside the rays (at most kMaxColumns - 2) -- every one comes back, and the
// caller's content goes in first where `in` is set.
template <typename Args>
struct RayCall {
    RmRays rays;
    Args args;
    hipError_t (*launch[2])(const RmRenderParams &, const RmRays &, const Args &, hipStream_t, const char **);
    int64_t chunk;
    int n_cols;
    Column cols[kMaxColumns];
    void column(const void *ptr, size_t bytes, void *slot, bool in, bool out = true) { cols[n_cols++] = Column{ptr, bytes, slot, in, out}; }
};

// Both forms of every ray query.  `check` makes the family's own checks, ahead of check_query like every argument check ahead of
// the device check; `describe` fills the family's RayCall once the arguments have passed.  The two forms are staged_call's,
// with the rays as two input columns; the host form takes finite rays only.  Nothing here depends on the family.
template <typename Args, typename Check, typename Describe>
int ray_call(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *origins, const void *dirs, bool host, void *stream, Check check,
             Describe describe) {
    if (!ctx) return RM_E_INVALID;
    int rc = check();
    if (!rc) rc = check_query(ctx, q, n, origins, dirs);
    if (rc || !n) return rc;
    const float *origins_xyz = static_cast<const float *>(origins), *dirs_xyz = static_cast<const float *>(dirs);
    if (host)
        for (int64_t i = 0; i < 3 * n; ++i)
            if (!std::isfinite(origins_xyz[i]) || !std::isfinite(dirs_xyz[i])) return fail(ctx, RM_E_INVALID, "non-finite ray");
    RmRenderParams p;
    rc = fill_query_params(ctx, q, p);
    if (rc) return rc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RayCall<Args> c{};
    c.column(origins, 12, &c.rays.origins, true, false);
    c.column(dirs, 12, &c.rays.dirs, true, false);
    describe(c);
    const auto launch = c.launch[ctx->opt_length ? 1 : 0];
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n, 1, c.chunk, c.cols, c.n_cols, [&](int64_t, int64_t m, hipStream_t s) {
        c.rays.n = m;
        return launch(p, c.rays, c.args, s, &ctx->last_kernel);
    });
}

int no_check() { return RM_OK; }  // rm_ray_march and rm_ray_pick have no checks of their own

// rm_ray_march (pick false: cast_kernel, no object column) and rm_ray_pick (pick true: pick_kernel)
void query_call(RayCall<RmQueryArgs> &c, const rm_ctx *ctx, const rm_ray_query *q, bool pick, void *t, void *iters, void *sdf_calls, void *normal,
                void *object) {
    c.launch[0] = pick ? rm_launch_pick : rm_launch_cast;
    c.launch[1] = pick ? rm_launch_pick_sqrt : rm_launch_cast_sqrt;
    c.chunk = kHostChunk;
    c.column(t, 8, &c.args.t, false);
    c.column(iters, 4, &c.args.iters, false);
    c.column(sdf_calls, 4, &c.args.sdf, false);
    c.column(normal, 12, &c.args.normal, false);
    if (pick) c.column(object, 4, &c.args.object, false);
    c.args.want_normal = q->normal != 0;
    c.args.slot_obj = ctx->dev.slot_object;
}

// what both forms of rm_ray_light check: the light
int check_light(rm_ctx *ctx, const rm_light *light) {
    if (!light) return fail(ctx, RM_E_INVALID, "null light");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(light->dir[k])) return fail(ctx, RM_E_INVALID, "non-finite light direction");
    if (light->ao_samples < 0 || light->ao_samples > 8) return fail(ctx, RM_E_INVALID, "ao_samples must be in [0, 8]");
    if (!std::isfinite(light->bias) || light->bias < 0) return fail(ctx, RM_E_INVALID, "bias must be finite and >= 0");
    if (!std::isfinite(light->ao_strength) || light->ao_strength < 0) return fail(ctx, RM_E_INVALID, "ao_strength must be finite and >= 0");
    if (!std::isfinite(light->ao_step) || (light->ao_samples > 0 && !(light->ao_step > 0)))
        return fail(ctx, RM_E_INVALID, "ao_step must be finite, and > 0 with occlusion samples");
    return RM_OK;
}

void light_call(RayCall<RmLightArgs> &c, const rm_light *light, void *t, void *iters, void *sdf_calls, void *normal, void *lit, void *ao, void *iters2,
                void *sdf_calls2) {
    c.launch[0] = rm_launch_light;
    c.launch[1] = rm_launch_light_sqrt;
    c.chunk = kHostChunk;
    c.column(t, 8, &c.args.t, false);
    c.column(iters, 4, &c.args.iters, false);
    c.column(sdf_calls, 4, &c.args.sdf, false);
    c.column(normal, 12, &c.args.normal, false);
    c.column(lit, 4, &c.args.lit, false);
    c.column(ao, 4, &c.args.ao, false);
    c.column(iters2, 4, &c.args.iters2, false);
    c.column(sdf_calls2, 4, &c.args.sdf2, false);
    c.args.bias = light->bias;
    c.args.ao_step = light->ao_step;
    c.args.ao_strength = light->ao_strength;
    std::memcpy(c.args.light, light->dir, sizeof c.args.light);
    c.args.ao_samples = light->ao_samples;
}

// what both forms of rm_ray_walk check: the record capacity and the outputs.  device: the caller's pointers are the kernel's,
// which stores records as 8-byte words (checked ahead of the rest).
static_assert(sizeof(rm_step) == 24 && sizeof(RmWalkStep) == 24 && sizeof(rm_walk) == 48 && sizeof(RmWalkSummary) == 48, "walk record layout");
static_assert(offsetof(rm_step, count) == offsetof(RmWalkStep, count) && offsetof(rm_walk, end) == offsetof(RmWalkSummary, end), "walk record layout");
static_assert(RM_END_HIT == 0 && RM_END_FAR == 1 && RM_END_STEPS == 2 && RM_END_ACCEL == 3 && RM_STEP_EVAL == 0 && RM_STEP_SKIP == 1,
              "the kernel's recorder writes these values");
int check_walk(rm_ctx *ctx, bool device, int64_t n, int32_t cap, const void *walks, const void *steps) {
    if (device && ((reinterpret_cast<uintptr_t>(walks) | reinterpret_cast<uintptr_t>(steps)) & 7u))
        return fail(ctx, RM_E_INVALID, "d_walks and d_steps must be 8-byte aligned");
    if (cap < 0 || cap > RM_WALK_MAX_STEPS) return fail(ctx, RM_E_INVALID, "cap must be in [0, RM_WALK_MAX_STEPS]");
    if (steps && cap == 0) return fail(ctx, RM_E_INVALID, "step records asked for with cap 0");
    if (n > 0 && !walks && !steps) return fail(ctx, RM_E_INVALID, "neither summaries nor step records asked for");
    return RM_OK;
}

// With step records the host form's chunk is sized by bytes: at most 64 MiB of records, at least one ray (cap 256: 10 922
// rays).  Slots past a ray's length are left as the caller has them: the caller's records go in, the kernel overwrites the
// ones the walk produced, and all come back.
void walk_call(RayCall<RmWalkArgs> &c, int32_t cap, void *walks, void *steps) {
    const size_t per_ray = sizeof(rm_step) * static_cast<size_t>(cap);
    c.launch[0] = rm_launch_walk;
    c.launch[1] = rm_launch_walk_sqrt;
    c.chunk = steps ? std::max<int64_t>(1, static_cast<int64_t>((size_t(64) << 20) / per_ray)) : kHostChunk;
    c.column(walks, sizeof(rm_walk), &c.args.walks, false);
    c.column(steps, per_ray, &c.args.steps, true);
    c.args.cap = cap;
}

// Object `index` of the active scene as an rm_scene_from_nodes forest (operands before their user, the object's root last),
// from the description the scene was built from: the upload as it was given (spheres as sphere leaves at
// SceneManager.getTransform of their centre), or the preset's objects as the reference holds them -- vec3 members
// (Box.halfSize, Repetition.spacing, AnimatedTranslate.direction) as their Float32Array values, operators with the
// Primitive.transform their constructors derive (wrappers: the operand's; unions: identity).  Unused operand indices are -1.
void object_forest(const rm_ctx *ctx, int index, std::vector<rm_node> &out) {
    out.clear();
    auto leaf = [&](int type, const float *m, const double *params, int n_params) {
        rm_node d;
        std::memset(&d, 0, sizeof d);
        d.type = type;
        d.child_a = d.child_b = -1;
        std::memcpy(d.world_to_local, m, sizeof d.world_to_local);
        for (int k = 0; k < n_params; ++k) d.params[k] = params[k];
        out.push_back(d);
    };
    auto sphere = [&](const float *c, double r) {
        float m[16];
        rmh::make_transform(c[0], c[1], c[2], nullptr, m);
        leaf(RM_PRIM_SPHERE, m, &r, 1);
    };
    auto forest = [&](const std::vector<rmh::NodeDesc> &nodes, int root, bool as_reference) {
        std::vector<std::array<float, 16>> T(nodes.size());  // Primitive.transform (rmh Forest::derive_transforms)
        for (size_t i = 0; i < nodes.size(); ++i) {
            const rmh::NodeDesc &d = nodes[i];
            if (d.type < 10 || !as_reference) std::memcpy(T[i].data(), d.m, sizeof d.m);
            else if (d.type == 11 || d.type == 12) T[i] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            else T[i] = T[d.a];
        }
        std::function<int(int)> emit = [&](int i) -> int {
            const rmh::NodeDesc &d = nodes[i];
            const bool binary = d.type == 11 || d.type == 12, op = d.type >= 10;
            const int a = op ? emit(d.a) : -1, b = binary ? emit(d.b) : -1;
            double p[6];
            for (int k = 0; k < 6; ++k) p[k] = d.params[k];
            if (as_reference && (d.type == 1 || d.type == 14 || d.type == 15))
                for (int k = 0; k < 3; ++k) p[k] = static_cast<float>(p[k]);
            leaf(d.type, T[i].data(), p, 6);
            out.back().child_a = a;
            out.back().child_b = b;
            return static_cast<int>(out.size()) - 1;
        };
        emit(root);
    };
    SceneDesc preset;
    const bool as_reference = !ctx->scene_is_uploaded;
    if (as_reference) {  // presets: as general primitive records where there are some (the sphere presets too), else as forests
        preset.kind = SceneDesc::kPrims;
        if (!rmh::preset_prims(ctx->scene_preset, preset.prims)) {
            preset.kind = SceneDesc::kNodes;
            if (!rmh::preset_nodes(ctx->scene_preset, preset.nodes, preset.roots)) return;
        }
    }
    const SceneDesc &d = as_reference ? preset : ctx->uploaded;
    switch (d.kind) {
        case SceneDesc::kSpheres: return sphere(&d.centers[3 * static_cast<size_t>(index)], d.radii[index]);
        case SceneDesc::kPrims: {
            rmh::PrimDesc pd = d.prims[index];
            if (as_reference && pd.type == RM_PRIM_BOX)
                for (double &v : pd.params) v = static_cast<float>(v);
            return leaf(pd.type, pd.m, pd.params, 3);
        }
        case SceneDesc::kNodes: return forest(d.nodes, d.roots[index], as_reference);
    }
}

// which rows of the job a render call renders: all of them, the stripes dealt round-robin to part `part` of `n_parts`
// (packed in increasing y), or the listed stripes (packed in list order)
struct Stripes {
    enum Kind { kWhole, kPart, kList } kind = kWhole;
    int32_t stripe_rows = 0, n_parts = 1, part = 0;
    const int32_t *ids = nullptr;
    int32_t n_ids = 0;
};

struct RenderBuffers {
    void *depth, *normal, *sdf, *iters, *rgba;
};

// The render entry behind rm_render_tile_device, rm_render_stripes_device and rm_render_stripe_list_device.  The accumulator
// of rm_render_attach_diagnostics is taken first, so every exit has consumed it (rm_raymarch.h: "whether it succeeds or
// not"); it reaches the launch as an argument.  A call whose rows come to none goes the way of every launch without pixels.
int render_device(rm_ctx *ctx, const rm_job *job, int32_t shader, const Stripes &s, const RenderBuffers &b, void *stream) {
    if (!ctx) return RM_E_INVALID;
    RmDiagDevice *diag = static_cast<RmDiagDevice *>(ctx->diag_next);
    ctx->diag_next = nullptr;
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU render path");
    int64_t mine = 0;  // rows of the stripes this call renders
    if (s.kind != Stripes::kWhole && !job) return fail(ctx, RM_E_INVALID, "null job");
    if (s.kind == Stripes::kPart) {
        mine = rm_stripe_rows(job->y_start, job->y_end, s.stripe_rows, s.n_parts, s.part);
        if (mine < 0) return fail(ctx, RM_E_INVALID, "bad stripe partition");
    }
    if (s.kind == Stripes::kList) {  // (refused before any scene work)
        if (s.stripe_rows <= 0 || s.n_ids < 0 || (s.n_ids > 0 && !s.ids)) return fail(ctx, RM_E_INVALID, "bad stripe list");
        const int64_t rows = job->y_end > job->y_start ? static_cast<int64_t>(job->y_end) - job->y_start : 0;
        const int64_t total = (rows + s.stripe_rows - 1) / s.stripe_rows;
        for (int k = 0; k < s.n_ids; ++k) {
            if (s.ids[k] < 0 || s.ids[k] >= total || (k > 0 && s.ids[k] <= s.ids[k - 1]))
                return fail(ctx, RM_E_INVALID, "stripe ids must be strictly increasing and inside the row range");
            const int64_t a = static_cast<int64_t>(s.ids[k]) * s.stripe_rows, e = a + s.stripe_rows;
            mine += (e < rows ? e : rows) - a;
        }
    }
    RmRenderParams p;
    int rc = fill_params(ctx, job, p);
    if (rc) return rc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    if (s.kind != Stripes::kWhole) {
        p.local_rows = static_cast<int32_t>(mine);
        p.stripe_rows = s.stripe_rows;
        p.n_parts = s.n_parts;
        p.part = s.part;
    }
    if (s.kind == Stripes::kList && mine > 0 && (rc = device_table(ctx, s.ids, static_cast<size_t>(s.n_ids), &p.stripe_ids))) return rc;
    p.shader = norm_shader(shader);
    p.depth = static_cast<uint8_t *>(b.depth);
    p.normal = static_cast<uint8_t *>(b.normal);
    p.sdf = static_cast<uint16_t *>(b.sdf);
    p.iters = static_cast<uint16_t *>(b.iters);
    p.rgba = static_cast<uint8_t *>(b.rgba);
    RM_HIP(ctx, launch_render(ctx, p, diag, static_cast<hipStream_t>(stream)));
    return RM_OK;
}

static_assert(sizeof(rm_compare_stats) == 128 && sizeof(RmCompareStats) == sizeof(rm_compare_stats) && sizeof(RmComparePartial) == 128,
              "compare_kernel writes rm_compare_stats records");
static_assert(RM_CMP_MAP_NONE == RM_CMP_NONE && RM_CMP_MAP_SDF == RM_CMP_SDF && RM_CMP_MAP_ITERS == RM_CMP_ITERS &&
              RM_CMP_MAP_DEPTH == RM_CMP_DEPTH && RM_CMP_MAP_NORMAL == RM_CMP_NORMAL && RM_CMP_MAP_SURFACE == RM_CMP_SURFACE,
              "compare_kernel's maps are rm_compare_map's");

// the checks both forms of rm_compare_frames make, ahead of the device check (the order of checks is behaviour)
int check_compare(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const rm_frame_set *a, const rm_frame_set *b, int32_t map,
                  int32_t gain, const void *rgba, const void *stats) {
    if (!a || !b) return fail(ctx, RM_E_INVALID, "null frame set");
    if (width < 0 || rows < 0 || n_frames < 0) return fail(ctx, RM_E_INVALID, "negative size");
    if (n_frames > 65535) return fail(ctx, RM_E_INVALID, "n_frames must be in [0, 65535] (one grid dimension)");
    if (!a->depth != !b->depth || !a->normal != !b->normal || !a->sdf != !b->sdf || !a->iters != !b->iters)
        return fail(ctx, RM_E_INVALID, "a buffer given on one side only");
    if (map < RM_CMP_MAP_NONE || map > RM_CMP_MAP_SURFACE) return fail(ctx, RM_E_INVALID, "unknown map");
    const void *of_map[] = {a->sdf, a->iters, a->depth, a->normal, a->normal};
    if (map != RM_CMP_MAP_NONE) {
        if (!of_map[map]) return fail(ctx, RM_E_INVALID, "the map's buffer is absent");
        if (gain < 1 || gain > 255) return fail(ctx, RM_E_INVALID, "gain must be in [1, 255]");
        if (!rgba) return fail(ctx, RM_E_INVALID, "a map needs an image buffer");
    }
    for (const void *p : {a->sdf, b->sdf, a->iters, b->iters})
        if (reinterpret_cast<uintptr_t>(p) & 1) return fail(ctx, RM_E_INVALID, "the counters must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats) & 7) return fail(ctx, RM_E_INVALID, "the records must be 8-byte aligned");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU compare path");
    return RM_OK;
}

static_assert(sizeof(struct rm_counter_hist) == 1064 && sizeof(rm_frame_hist) == 2128 && sizeof(RmCounterHist) == sizeof(struct rm_counter_hist) &&
                  sizeof(RmFrameHist) == sizeof(rm_frame_hist) && RM_HIST_NBINS == RM_HIST_BINS && sizeof(RmHistScratch) == 2096,
              "hist_kernel writes rm_frame_hist records");

// what both forms of rm_counter_hist and of rm_shade_ranged check about the frames, ahead of the device check
int check_frames(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames) {
    if (width < 0 || rows < 0 || n_frames < 0) return fail(ctx, RM_E_INVALID, "negative size");
    if (static_cast<uint64_t>(width) * static_cast<uint64_t>(rows) > UINT32_MAX) return fail(ctx, RM_E_INVALID, "more than UINT32_MAX pixels per frame");
    if (n_frames > 65535) return fail(ctx, RM_E_INVALID, "n_frames must be in [0, 65535] (one grid dimension)");
    return RM_OK;
}

int check_hist(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const void *sdf, const void *iters, const void *normal, int32_t mask,
               int32_t bin_shift, int32_t lo_permille, int32_t hi_permille, const void *hist) {
    if (!hist) return fail(ctx, RM_E_INVALID, "null records");
    if (!sdf && !iters) return fail(ctx, RM_E_INVALID, "both counters are absent");
    if (const int rc = check_frames(ctx, width, rows, n_frames)) return rc;
    if (mask < RM_HIST_ALL || mask > RM_HIST_BACKGROUND) return fail(ctx, RM_E_INVALID, "unknown mask");
    if (mask != RM_HIST_ALL && !normal) return fail(ctx, RM_E_INVALID, "the mask needs the normal buffer");
    if (bin_shift < 0 || bin_shift > 8) return fail(ctx, RM_E_INVALID, "bin_shift must be in [0, 8]");
    if (lo_permille < 0 || lo_permille > hi_permille || hi_permille > 1000) return fail(ctx, RM_E_INVALID, "need 0 <= lo_permille <= hi_permille <= 1000");
    if ((reinterpret_cast<uintptr_t>(sdf) | reinterpret_cast<uintptr_t>(iters)) & 1) return fail(ctx, RM_E_INVALID, "the counters must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(hist) & 7) return fail(ctx, RM_E_INVALID, "the records must be 8-byte aligned");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU histogram path");
    return RM_OK;
}

int check_shade_ranged(rm_ctx *ctx, int32_t counter, int32_t width, int32_t rows, int32_t n_frames, const void *values, const void *hist,
                       uint32_t lo, uint32_t hi, const void *rgba) {
    if (!rgba) return fail(ctx, RM_E_INVALID, "null image");
    if (!values) return fail(ctx, RM_E_INVALID, "null counter buffer");
    if (counter != 0 && counter != 1) return fail(ctx, RM_E_INVALID, "counter must be 0 (sdf) or 1 (iters)");
    if (const int rc = check_frames(ctx, width, rows, n_frames)) return rc;
    if (!hist && lo > hi) return fail(ctx, RM_E_INVALID, "lo > hi");
    if (reinterpret_cast<uintptr_t>(values) & 1) return fail(ctx, RM_E_INVALID, "the counter must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(hist) & 7) return fail(ctx, RM_E_INVALID, "the records must be 8-byte aligned");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU shading path");
    return RM_OK;
}

int check_shade_lit(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const void *depth, const void *normal, const void *lit,
                    const void *ao, const void *rgba) {
    if (!depth || !normal || !lit || !ao || !rgba) return fail(ctx, RM_E_INVALID, "null buffer");
    if (const int rc = check_frames(ctx, width, rows, n_frames)) return rc;
    if ((reinterpret_cast<uintptr_t>(lit) | reinterpret_cast<uintptr_t>(ao)) & 3) return fail(ctx, RM_E_INVALID, "lit and ao must be 4-byte aligned");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU shading path");
    return RM_OK;
}

// ---- field queries: the lattice, its checks and the two kernels' arguments

static_assert(sizeof(rm_lattice) == 72 && sizeof(rm_field_shade) == 40, "field query layout");
static_assert(RM_FIELD_MAP_DISTANCE == 0 && RM_FIELD_MAP_COUNT == 1, "shade_field_kernel reads these values");

// component c of lattice point (i, j, k): binary64, left to right, one rounding (the header's rule; field_kernel forms the same)
float lattice_component(const rm_lattice &l, int c, int64_t i, int64_t j, int64_t k) {
    return static_cast<float>(((static_cast<double>(l.origin[c]) + static_cast<double>(i) * static_cast<double>(l.du[c])) +
                               static_cast<double>(j) * static_cast<double>(l.dv[c])) +
                              static_cast<double>(k) * static_cast<double>(l.dw[c]));
}

// null when the lattice is well formed (then *n = nu * nv * nw), else what is wrong with it
const char *lattice_error(const rm_lattice *l, int64_t *n) {
    if (!l) return "null lattice";
    if (l->nu < 0 || l->nu > 65535 || l->nv < 0 || l->nv > 65535 || l->nw < 0 || l->nw > 65535) return "lattice counts must be in [0, 65535]";
    if (l->reserved != 0) return "rm_lattice.reserved must be 0";
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(l->origin[c]) || !std::isfinite(l->du[c]) || !std::isfinite(l->dv[c]) || !std::isfinite(l->dw[c])) return "non-finite lattice vector";
    if (!std::isfinite(l->time)) return "non-finite time";
    // every component is monotone in each index: the eight corners (indices 0 and count - 1; 0 for an empty axis) bound all points
    const int64_t last[3] = {l->nu > 0 ? l->nu - 1 : 0, l->nv > 0 ? l->nv - 1 : 0, l->nw > 0 ? l->nw - 1 : 0};
    for (int corner = 0; corner < 8; ++corner)
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(lattice_component(*l, c, corner & 1 ? last[0] : 0, corner & 2 ? last[1] : 0, corner & 4 ? last[2] : 0)))
                return "a lattice corner is not a finite binary32 point";
    *n = static_cast<int64_t>(l->nu) * l->nv * l->nw;
    return nullptr;
}

// what both forms of rm_scene_field check, arguments first; *n receives the point count
int check_field(rm_ctx *ctx, const rm_lattice *lat, const void *dist, const void *dist32, const void *count, int64_t *n) {
    if (const char *bad = lattice_error(lat, n)) return fail(ctx, RM_E_INVALID, bad);
    if (reinterpret_cast<uintptr_t>(dist) & 7) return fail(ctx, RM_E_INVALID, "dist must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(dist32) | reinterpret_cast<uintptr_t>(count)) & 3) return fail(ctx, RM_E_INVALID, "dist32 and count must be 4-byte aligned");
    if (*n > 0 && !dist && !dist32 && !count) return fail(ctx, RM_E_INVALID, "no output asked for");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU distance path");
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    return RM_OK;
}

// The lattice as the kernels take it: the binary32 vectors widened (exact).  Every argument block that names a lattice opens with it.
RmLattice widen_lattice(const rm_lattice &l) {
    RmLattice w;
    for (int c = 0; c < 3; ++c) {
        w.origin[c] = l.origin[c];
        w.du[c] = l.du[c];
        w.dv[c] = l.dv[c];
        w.dw[c] = l.dw[c];
    }
    return w;
}

// The parameter block and the lattice of a field query: the active scene at the lattice's own time (fill_scene_query).
void fill_field(const rm_ctx *ctx, const rm_lattice *lat, RmRenderParams &p, RmFieldArgs &a) {
    fill_scene_query(ctx, lat->time, p);
    std::memset(&a, 0, sizeof a);
    a.lat = widen_lattice(*lat);
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
}

// ---- meshes: surface nets over a lattice of values (rm_mesh.hip)

static_assert(sizeof(rm_mesh_info) == 32 && sizeof(RmMeshInfo) == sizeof(rm_mesh_info), "rm_mesh_info layout");
static_assert(RM_MESH_F64 == 0 && RM_MESH_F32 == 1, "rm_launch_mesh reads these values");

// Where a mesh launch writes: device pointers for the kernels, the caller's host pointers in a host entry.  cells and edges are
// the sparse mesher's keys (null: not asked for; the dense entries have none).
struct MeshOutputs {
    void *vertices, *quads, *cells, *edges, *info;
    int64_t cap_vertices, cap_quads;
};

// What both mesh entries check, arguments first, each described once; *n receives the point count and *cells whether the
// lattice has a cell (every count at least 2).  `values` null: the entry samples the scene itself (rm_scene_mesh) and needs one.
struct MeshCall {
    const rm_lattice *lattice;
    bool own_values;  // rm_mesh_field_device: d_values and value_type are arguments
    const void *values;
    int32_t value_type;
    double iso;
    MeshOutputs out;
};

bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// what every mesh entry, dense or sparse, checks about iso, capacities and output buffers (the sparse ones: cells and edges too)
const char *mesh_outputs_error(double iso, const MeshOutputs &o) {
    if (!std::isfinite(iso)) return "non-finite iso";
    if (o.cap_vertices < 0 || o.cap_quads < 0) return "negative capacity";
    if ((o.cap_vertices > 0 && !o.vertices) || (o.cap_quads > 0 && !o.quads)) return "null buffer with a capacity above 0";
    if (misaligned(o.vertices, 3) || misaligned(o.quads, 3)) return "vertices and quads must be 4-byte aligned";
    if (misaligned(o.cells, 7) || misaligned(o.edges, 7)) return "cells and edges must be 8-byte aligned";
    return nullptr;
}

// what an entry without a host path asks of the context, behind its arguments: a device (no CPU `path`), then a scene if it samples one
int need_device(rm_ctx *ctx, const char *path, bool scene) {
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, std::string("host-only context: there is no CPU ") + path);
    if (scene && !ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    return RM_OK;
}

int check_mesh(rm_ctx *ctx, const MeshCall &m, int64_t *n, bool *cells) {
    if (const char *bad = lattice_error(m.lattice, n)) return fail(ctx, RM_E_INVALID, bad);
    if (*n > (int64_t(1) << 30)) return fail(ctx, RM_E_INVALID, "more than 2^30 lattice points: the mesher does not split a volume");
    *cells = m.lattice->nu >= 2 && m.lattice->nv >= 2 && m.lattice->nw >= 2;
    if (!m.out.info) return fail(ctx, RM_E_INVALID, "null info");
    if (const char *bad = mesh_outputs_error(m.iso, m.out)) return fail(ctx, RM_E_INVALID, bad);
    if (m.own_values) {
        if (m.value_type != RM_MESH_F64 && m.value_type != RM_MESH_F32) return fail(ctx, RM_E_INVALID, "value_type must be RM_MESH_F64 or RM_MESH_F32");
        if (*cells && !m.values) return fail(ctx, RM_E_INVALID, "null values");
        if (reinterpret_cast<uintptr_t>(m.values) & (m.value_type == RM_MESH_F64 ? 7 : 3)) return fail(ctx, RM_E_INVALID, "values must be aligned to their type");
        if (reinterpret_cast<uintptr_t>(m.out.info) & 7) return fail(ctx, RM_E_INVALID, "info must be 8-byte aligned");
    }
    return need_device(ctx, "mesher", !m.own_values);
}

// the outputs and the mesher's scratch of an argument block, dense or sparse
template <typename ARGS>
void fill_mesh_outputs(ARGS &a, const MeshOutputs &o, uint32_t *d_map, uint32_t *d_totals) {
    a.vertices = static_cast<float *>(o.vertices);
    a.quads = static_cast<uint32_t *>(o.quads);
    a.info = static_cast<RmMeshInfo *>(o.info);
    a.map = d_map;
    a.totals = d_totals;
    a.cap_vertices = o.cap_vertices;
    a.cap_quads = o.cap_quads;
}

// The launch both entries share: m.values laid out by the lattice, m.out and the values on the device, the map and the block
// totals at their places in the reserved scratch.
RmMeshArgs mesh_args(const Staging &st, const MeshCall &m, int64_t n, size_t o_map, size_t o_totals) {
    RmMeshArgs a;
    std::memset(&a, 0, sizeof a);
    a.lat = widen_lattice(*m.lattice);
    a.values = m.values;
    a.iso = m.iso;
    fill_mesh_outputs(a, m.out, st.at<uint32_t>(o_map), st.at<uint32_t>(o_totals));
    a.n = n;
    a.nu = static_cast<unsigned int>(m.lattice->nu);
    a.nv = static_cast<unsigned int>(m.lattice->nv);
    a.nw = static_cast<unsigned int>(m.lattice->nw);
    a.n_blocks = static_cast<unsigned int>((n + RM_MESH_BLOCK - 1) / RM_MESH_BLOCK);
    a.f32 = m.value_type == RM_MESH_F32;
    return a;
}

int launch_mesh(rm_ctx *ctx, const Staging &st, const MeshCall &m, int64_t n, size_t o_map, size_t o_totals, hipStream_t stream) {
    RM_HIP(ctx, rm_launch_mesh(mesh_args(st, m, n, o_map, o_totals), stream, &ctx->last_kernel));
    return RM_OK;
}

size_t mesh_blocks(int64_t n) { return static_cast<size_t>((n + RM_MESH_BLOCK - 1) / RM_MESH_BLOCK); }

// The outputs of a host mesh entry in the scratch buffer, behind the entry's other regions: the info, then room for what the
// caller's capacities hold or the lattice or the kept blocks can yield at most, whichever is less; keys only where asked for.
struct MeshRegions {
    size_t room_v, room_q, o_info, o_vert, o_quad, o_cells, o_edges;
    MeshRegions(Staging &st, const MeshOutputs &host, int64_t most_v, int64_t most_q)
        : room_v(static_cast<size_t>(std::min(host.cap_vertices, most_v))), room_q(static_cast<size_t>(std::min(host.cap_quads, most_q))),
          o_info(st.region(sizeof(rm_mesh_info))), o_vert(st.region(12 * room_v)), o_quad(st.region(16 * room_q)),
          o_cells(st.region(host.cells ? 8 * room_v : 0)), o_edges(st.region(host.edges ? 8 * room_q : 0)) {}
    // the same outputs as the kernels see them, once the scratch is reserved
    MeshOutputs on_device(const Staging &st, const MeshOutputs &host) const {
        return {st.at<void>(o_vert), st.at<void>(o_quad), host.cells ? st.at<void>(o_cells) : nullptr, host.edges ? st.at<void>(o_edges) : nullptr,
                st.at<void>(o_info), static_cast<int64_t>(room_v), static_cast<int64_t>(room_q)};
    }
};

// How both host mesh entries end: the info comes back first, then of every output asked for what the mesher wrote of it --
// min(info->n_vertices, room_v) records per vertex, min(info->n_quads, room_q) per quad.
int read_mesh(rm_ctx *ctx, const Staging &st, const MeshRegions &r, const MeshOutputs &host) {
    rm_mesh_info *info = static_cast<rm_mesh_info *>(host.info);
    RM_HIP(ctx, st.out(info, r.o_info, sizeof *info));
    RM_HIP(ctx, st.sync());
    const size_t got_v = static_cast<size_t>(std::min<int64_t>(info->n_vertices, static_cast<int64_t>(r.room_v))),
                 got_q = static_cast<size_t>(std::min<int64_t>(info->n_quads, static_cast<int64_t>(r.room_q)));
    const struct {
        void *host;  // null: not asked for
        size_t offset, bytes;
    } outputs[] = {{host.vertices, r.o_vert, 12 * got_v}, {host.quads, r.o_quad, 16 * got_q}, {host.cells, r.o_cells, 8 * got_v}, {host.edges, r.o_edges, 8 * got_q}};
    for (const auto &o : outputs)
        if (o.bytes && o.host) RM_HIP(ctx, st.out(o.host, o.offset, o.bytes));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

// ---- sparse meshes: blocks of 8 x 8 x 8 cells, their tiles and the mesher over them (rm_kernels.hip, rm_mesh_sparse.hip)

static_assert(sizeof(rm_sparse_info) == 32 && sizeof(RmSparseInfo) == sizeof(rm_sparse_info), "rm_sparse_info layout");

struct SparseGrid {
    int64_t n;         // lattice points
    int32_t nb[3];     // blocks per axis
    int64_t n_blocks;
};

// null when the lattice is well formed and has at most 2^24 blocks (then *g is filled), else what is wrong with it
const char *sparse_error(const rm_lattice *l, SparseGrid *g, bool limit = true) {
    if (const char *bad = lattice_error(l, &g->n)) return bad;
    const int32_t count[3] = {l->nu, l->nv, l->nw};
    for (int c = 0; c < 3; ++c) g->nb[c] = count[c] >= 2 ? (count[c] - 1 + RM_SPARSE_BLOCK - 1) / RM_SPARSE_BLOCK : 0;
    g->n_blocks = static_cast<int64_t>(g->nb[0]) * g->nb[1] * g->nb[2];
    if (limit && g->n_blocks > RM_SPARSE_MAX_BLOCKS) return "more than 2^24 blocks";
    return nullptr;
}

// What the sparse entries check about the kept blocks, in two parts because two of the three entries check other arguments in
// between: n_kept in [0, min(n_blocks, cap)] (cap 0: none), and the list and the tiles once a block is kept.
static_assert(RM_SPARSE_MAX_KEPT == 1 << 21, "the text of kept_range_error");
const char *kept_range_error(const SparseGrid &g, int64_t n_kept, int64_t cap = 0) {
    if (n_kept < 0 || n_kept > g.n_blocks || (cap && n_kept > cap)) return cap ? "n_kept must be in [0, min(n_blocks, 2^21)]" : "n_kept must be in [0, n_blocks]";
    return nullptr;
}
const char *kept_buffers_error(int64_t n_kept, const void *list, const void *tiles) {
    return n_kept > 0 && (!list || !tiles) ? "null list or tiles" : nullptr;
}

// lipschitz * R + slack of the header's rule, one binary64 operation at a time
double sparse_bound(const rm_lattice &l, double lipschitz) {
    const auto norm = [](const float v[3]) {
        const double x = v[0], y = v[1], z = v[2];
        return std::sqrt((x * x + y * y) + z * z);
    };
    const double R = 4.0 * ((norm(l.du) + norm(l.dv)) + norm(l.dw));
    const int64_t last[3] = {l.nu > 0 ? l.nu - 1 : 0, l.nv > 0 ? l.nv - 1 : 0, l.nw > 0 ? l.nw - 1 : 0};
    double M = 0.0;
    for (int corner = 0; corner < 8; ++corner)
        for (int c = 0; c < 3; ++c)
            M = std::max(M, std::fabs(static_cast<double>(lattice_component(l, c, corner & 1 ? last[0] : 0, corner & 2 ? last[1] : 0, corner & 4 ? last[2] : 0))));
    const double slack = M * 0x1p-20;
    return lipschitz * R + slack;
}

template <typename ARGS>
void fill_sparse_lattice(const rm_lattice *lat, const SparseGrid &g, ARGS &a) {
    std::memset(&a, 0, sizeof a);
    a.lat = widen_lattice(*lat);
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
    a.nw = static_cast<unsigned int>(lat->nw);
    a.nbu = static_cast<unsigned int>(g.nb[0]);
    a.nbv = static_cast<unsigned int>(g.nb[1]);
}

size_t sparse_groups(int64_t n_blocks) { return static_cast<size_t>((n_blocks + 255) / 256); }

// The three launches; every pointer a device pointer, the scene the active one at the lattice's time.
int launch_blocks(rm_ctx *ctx, const rm_lattice *lat, const SparseGrid &g, double iso, double lipschitz, void *d_slot, void *d_list, void *d_dist,
                  void *d_info, uint32_t *d_totals, hipStream_t stream) {
    RmRenderParams p;
    fill_scene_query(ctx, lat->time, p);
    RmBlocksArgs a;
    fill_sparse_lattice(lat, g, a);
    a.nbw = static_cast<unsigned int>(g.nb[2]);
    a.iso = iso;
    a.bound = sparse_bound(*lat, lipschitz);
    a.slot = static_cast<int32_t *>(d_slot);
    a.list = static_cast<int32_t *>(d_list);
    a.dist = static_cast<double *>(d_dist);
    a.info = static_cast<RmSparseInfo *>(d_info);
    a.totals = d_totals;
    a.n_blocks = static_cast<unsigned int>(g.n_blocks);
    a.n_groups = static_cast<unsigned int>(sparse_groups(g.n_blocks));
    RM_HIP(ctx, (ctx->opt_length ? rm_launch_blocks_sqrt : rm_launch_blocks)(p, a, stream, &ctx->last_kernel));
    return RM_OK;
}

// The argument block of a tile launch, the full one and the update
RmTilesArgs tiles_args(const rm_lattice *lat, const SparseGrid &g, const void *d_list, int64_t n_kept, void *d_tiles) {
    RmTilesArgs a;
    fill_sparse_lattice(lat, g, a);
    // read by the exact launch only: the coarse pass's bound for a 1-Lipschitz field, and per axis the same four steps and slack
    a.radius = sparse_bound(*lat, 1.0);
    const double slack = sparse_bound(*lat, 0.0);
    for (int c = 0; c < 3; ++c)
        a.half[c] = 4.0 * ((std::fabs(static_cast<double>(lat->du[c])) + std::fabs(static_cast<double>(lat->dv[c]))) + std::fabs(static_cast<double>(lat->dw[c]))) + slack;
    a.list = static_cast<const int32_t *>(d_list);
    a.tiles = static_cast<double *>(d_tiles);
    a.n_kept = static_cast<unsigned int>(n_kept);
    return a;
}

// exact: the exact field whatever option `exact` says (rm_scene_measure)
int launch_tiles(rm_ctx *ctx, const rm_lattice *lat, const SparseGrid &g, const void *d_list, int64_t n_kept, void *d_tiles, hipStream_t stream,
                 bool exact = false) {
    RmRenderParams p;
    fill_scene_query(ctx, lat->time, p);
    if (const int erc = exact ? use_exact(ctx, p) : apply_exact(ctx, p)) return erc;
    const RmTilesArgs a = tiles_args(lat, g, d_list, n_kept, d_tiles);
    RM_HIP(ctx, (ctx->opt_length ? rm_launch_tiles_sqrt : rm_launch_tiles)(p, a, stream, &ctx->last_kernel));
    return RM_OK;
}

// rm_scene_tiles_update_device: the exact tile launch with a previous scene's tiles to copy from (rm_kernels.hip,
// tiles_update_kernel) and, where flags are written, their totals.
struct TilesUpdateCall {
    const void *prev_slot, *prev_tiles, *balls;
    int64_t n_prev_kept;
    int32_t n_balls;
    void *reused, *info;  // reused: the caller's flags or scratch, null when neither flags nor totals are asked for
};
int launch_tiles_update(rm_ctx *ctx, const rm_lattice *lat, const SparseGrid &g, const TilesUpdateCall &c, const void *d_list, int64_t n_kept,
                        void *d_tiles, hipStream_t stream) {
    RmRenderParams p;
    fill_scene_query(ctx, lat->time, p);
    if (const int erc = use_exact(ctx, p)) return erc;
    const RmTilesArgs a = tiles_args(lat, g, d_list, n_kept, d_tiles);
    RmTilesUpdateArgs u;
    std::memset(&u, 0, sizeof u);
    u.prev_slot = static_cast<const int32_t *>(c.prev_slot);
    u.prev_tiles = static_cast<const double *>(c.prev_tiles);
    u.balls = static_cast<const RmBall *>(c.balls);
    u.reused = static_cast<int32_t *>(c.reused);
    u.n_blocks = static_cast<unsigned int>(g.n_blocks);
    u.n_prev_kept = static_cast<unsigned int>(c.n_prev_kept);
    u.n_balls = c.n_balls;
    RM_HIP(ctx, (ctx->opt_length ? rm_launch_tiles_update_sqrt : rm_launch_tiles_update)(p, a, u, stream, &ctx->last_kernel));
    if (c.info) RM_HIP(ctx, rm_launch_tiles_update_totals(u.reused, a.n_kept, static_cast<RmTilesUpdateInfo *>(c.info), stream));
    return RM_OK;
}

struct SparseMeshCall {
    const void *slot, *list, *tiles;
    int64_t n_kept;
    double iso;
    MeshOutputs out;
};

int launch_mesh_tiles(rm_ctx *ctx, const rm_lattice *lat, const SparseGrid &g, const SparseMeshCall &m, uint32_t *d_map, uint32_t *d_totals,
                      hipStream_t stream) {
    RmSparseMeshArgs a;
    fill_sparse_lattice(lat, g, a);
    a.nbw = static_cast<unsigned int>(g.nb[2]);
    a.iso = m.iso;
    a.slot = static_cast<const int32_t *>(m.slot);
    a.list = static_cast<const int32_t *>(m.list);
    a.tiles = static_cast<const double *>(m.tiles);
    fill_mesh_outputs(a, m.out, d_map, d_totals);
    a.cells = static_cast<long long *>(m.out.cells);
    a.edges = static_cast<long long *>(m.out.edges);
    a.n_kept = static_cast<unsigned int>(m.n_kept);
    RM_HIP(ctx, rm_launch_mesh_tiles(a, stream, &ctx->last_kernel));
    return RM_OK;
}

// ---- measures: integer sums over the inside points of a lattice (rm_measure.hip)

static_assert(sizeof(rm_measure) == 176 && sizeof(RmMeasure) == sizeof(rm_measure) && offsetof(rm_measure, lo) == 120 &&
                  offsetof(rm_measure, n_blocks) == 144 && offsetof(RmMeasure, n_blocks) == 144,
              "rm_measure layout");
static_assert(sizeof(struct rm_measure_world) == 120 && sizeof(RmMeasurePartial) == 144, "rm_measure_world and partial layout");

// every sum of a measure fits an int64: n * (max(nu, nv, nw) - 1)^2 stays below 2^63 (formed without overflow)
bool measure_fits(const rm_lattice &l, int64_t n) {
    const int64_t m = std::max(std::max(l.nu, l.nv), l.nw) - 1;
    return m <= 0 || n <= std::numeric_limits<int64_t>::max() / (m * m);
}
const char *const kMeasureOverflow = "the sums of this lattice do not fit 64 bits: n_points * (max count - 1)^2 reaches 2^63";

// The dense launch: the values and the record on the device, the partials at their place in the reserved scratch.
int launch_measure_field(rm_ctx *ctx, const rm_lattice *lat, int64_t n, const void *d_values, int32_t value_type, double iso, void *d_partials,
                         unsigned int n_groups, void *d_measure, hipStream_t stream) {
    RmMeasureFieldArgs a;
    std::memset(&a, 0, sizeof a);
    a.values = d_values;
    a.iso = iso;
    a.partials = static_cast<RmMeasurePartial *>(d_partials);
    a.out = static_cast<RmMeasure *>(d_measure);
    a.n = n;
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
    a.nw = static_cast<unsigned int>(lat->nw);
    a.f32 = value_type == RM_MESH_F32;
    RM_HIP(ctx, rm_launch_measure_field(a, n_groups, stream, &ctx->last_kernel));
    return RM_OK;
}

struct SparseMeasureCall {
    const void *slot, *list, *dist, *tiles;
    int64_t n_kept;
    double iso;
    void *measure;
};

int launch_measure_tiles(rm_ctx *ctx, const rm_lattice *lat, const SparseGrid &g, const SparseMeasureCall &m, void *d_partials, unsigned int n_groups,
                         hipStream_t stream) {
    RmMeasureTilesArgs a;
    std::memset(&a, 0, sizeof a);
    a.iso = m.iso;
    a.slot = static_cast<const int32_t *>(m.slot);
    a.list = static_cast<const int32_t *>(m.list);
    a.dist = static_cast<const double *>(m.dist);
    a.tiles = static_cast<const double *>(m.tiles);
    a.partials = static_cast<RmMeasurePartial *>(d_partials);
    a.out = static_cast<RmMeasure *>(m.measure);
    a.n = g.n;
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
    a.nw = static_cast<unsigned int>(lat->nw);
    a.nbu = static_cast<unsigned int>(g.nb[0]);
    a.nbv = static_cast<unsigned int>(g.nb[1]);
    a.nbw = static_cast<unsigned int>(g.nb[2]);
    a.n_blocks = static_cast<unsigned int>(g.n_blocks);
    a.n_kept = static_cast<unsigned int>(m.n_kept);
    RM_HIP(ctx, rm_launch_measure_tiles(a, n_groups, stream, &ctx->last_kernel));
    return RM_OK;
}

// what the sparse measure entries ask of the lattice beyond sparse_error: blocks on every axis
const char *measure_blocks_error(const rm_lattice *l) {
    return l->nu < 2 || l->nv < 2 || l->nw < 2 ? "every lattice count must be at least 2: a slice goes through rm_measure_field_device" : nullptr;
}

int check_shade_field(rm_ctx *ctx, const rm_field_shade *sh, int64_t n, const void *values, const void *rgba) {
    if (!sh || !values || !rgba) return fail(ctx, RM_E_INVALID, "null argument");
    if (n < 0) return fail(ctx, RM_E_INVALID, "negative count");
    if (sh->map != RM_FIELD_MAP_DISTANCE && sh->map != RM_FIELD_MAP_COUNT) return fail(ctx, RM_E_INVALID, "map must be RM_FIELD_MAP_DISTANCE or RM_FIELD_MAP_COUNT");
    if (sh->reserved != 0) return fail(ctx, RM_E_INVALID, "rm_field_shade.reserved must be 0");
    if (sh->map == RM_FIELD_MAP_DISTANCE) {
        if (!std::isfinite(sh->range) || !(sh->range > 0) || !std::isfinite(sh->band) || !(sh->band > 0)) return fail(ctx, RM_E_INVALID, "range and band must be finite and positive");
        if (!std::isfinite(sh->line) || sh->line < 0) return fail(ctx, RM_E_INVALID, "line must be finite and not negative");
        if (reinterpret_cast<uintptr_t>(values) & 7) return fail(ctx, RM_E_INVALID, "distances must be 8-byte aligned");
    } else {
        if (sh->lo > sh->hi) return fail(ctx, RM_E_INVALID, "lo > hi");
        if (reinterpret_cast<uintptr_t>(values) & 3) return fail(ctx, RM_E_INVALID, "counts must be 4-byte aligned");
    }
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU shading path");
    return RM_OK;
}

// rm_scene_distance and rm_debug_wave_distance: n finite host points through the scratch buffer, synchronous.  `ready` runs
// behind the argument checks and ahead of any device call and may refuse the call; `launch` enqueues the kernel on the
// context's stream for the staged points and outputs.
template <typename Ready, typename Launch>
int points_call(rm_ctx *ctx, const float *points_xyz, int64_t n, double *dist, uint32_t *count, Ready ready, Launch launch) {
    RM_NEED_DEVICE(ctx, "host-only context");
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    if (n < 0 || (n > 0 && (!points_xyz || !dist || !count))) return fail(ctx, RM_E_INVALID, "bad buffers");
    if (!n) return RM_OK;
    for (int64_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(points_xyz[i])) return fail(ctx, RM_E_INVALID, "non-finite point");
    int rc = ready();
    if (rc) return rc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t k = static_cast<size_t>(n);
    Staging st{ctx};
    const size_t o_pts = st.region(12 * k), o_dist = st.region(8 * k), o_cnt = st.region(4 * k);
    if ((rc = st.reserve())) return rc;
    RM_HIP(ctx, st.in(o_pts, points_xyz, 12 * k));
    RM_HIP(ctx, launch(st.at<const float>(o_pts), st.at<double>(o_dist), st.at<uint32_t>(o_cnt)));
    RM_HIP(ctx, st.out(dist, o_dist, 8 * k));
    RM_HIP(ctx, st.out(count, o_cnt, 4 * k));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

// ---- point queries (rm_scene_points)

static_assert(sizeof(rm_point_query) == 40, "rm_point_query layout");

// what both forms of rm_scene_points check, arguments first; host: the points are the caller's host buffer and must be finite
int check_points(rm_ctx *ctx, const rm_point_query *q, int64_t n, const float *points, bool host, const void *position, const void *dist,
                 const void *normal, const void *object, const void *steps, const void *count) {
    if (!q) return fail(ctx, RM_E_INVALID, "null query");
    if (q->reserved[0] != 0 || q->reserved[1] != 0) return fail(ctx, RM_E_INVALID, "rm_point_query.reserved must be 0");
    if (q->flags & ~RM_POINT_NORMAL) return fail(ctx, RM_E_INVALID, "unknown flag bits");
    if (q->snap_steps < 0 || q->snap_steps > 16) return fail(ctx, RM_E_INVALID, "snap_steps must be in [0, 16]");
    if (!std::isfinite(q->time) || !std::isfinite(q->iso) || !std::isfinite(q->snap_tol)) return fail(ctx, RM_E_INVALID, "non-finite time, iso or snap_tol");
    if (q->snap_tol < 0) return fail(ctx, RM_E_INVALID, "snap_tol must be >= 0");
    if (n < 0 || n > std::numeric_limits<int32_t>::max()) return fail(ctx, RM_E_INVALID, "point count out of range");
    if (n > 0 && !points) return fail(ctx, RM_E_INVALID, "null point buffer");
    if (n > 0 && !position && !dist && !normal && !object && !steps && !count) return fail(ctx, RM_E_INVALID, "no output asked for");
    if (reinterpret_cast<uintptr_t>(dist) & 7) return fail(ctx, RM_E_INVALID, "dist must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(position) | reinterpret_cast<uintptr_t>(normal) | reinterpret_cast<uintptr_t>(object) | reinterpret_cast<uintptr_t>(steps) |
         reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(points)) & 3)
        return fail(ctx, RM_E_INVALID, "points, position, normal, object, steps and count must be 4-byte aligned");
    if (host)
        for (int64_t i = 0; i < 3 * n; ++i)
            if (!std::isfinite(points[i])) return fail(ctx, RM_E_INVALID, "non-finite point");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU distance path");
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    return RM_OK;
}

// The parameter block and the query of a point query: the active scene at the query's own time (fill_scene_query).
void fill_points(const rm_ctx *ctx, const rm_point_query *q, RmRenderParams &p, RmPointArgs &a) {
    fill_scene_query(ctx, q->time, p);
    std::memset(&a, 0, sizeof a);
    a.slot_obj = ctx->dev.slot_object;
    a.iso = q->iso;
    a.snap_tol = q->snap_tol;
    a.snap_steps = q->snap_steps;
    a.want_normal = (q->flags & RM_POINT_NORMAL) ? 1 : 0;
}

// ---- sharp vertices (rm_scene_sharpen)

static_assert(sizeof(rm_sharp_query) == 32, "rm_sharp_query layout");

// what both forms of rm_scene_sharpen check, arguments first
int check_sharp(rm_ctx *ctx, const rm_lattice *lat, const rm_sharp_query *q, int64_t n, const void *cells, const void *position, const void *feature,
                const void *count) {
    int64_t points = 0;
    if (const char *bad = lattice_error(lat, &points)) return fail(ctx, RM_E_INVALID, bad);
    if (!q) return fail(ctx, RM_E_INVALID, "null query");
    if (q->reserved != 0) return fail(ctx, RM_E_INVALID, "rm_sharp_query.reserved must be 0");
    if (q->refine < 0 || q->refine > 8) return fail(ctx, RM_E_INVALID, "refine must be in [0, 8]");
    if (!std::isfinite(q->iso)) return fail(ctx, RM_E_INVALID, "non-finite iso");
    if (!(q->rank_tol >= 0 && q->rank_tol <= 1)) return fail(ctx, RM_E_INVALID, "rank_tol must be in [0, 1]");
    if (!std::isfinite(q->reach) || q->reach < 0) return fail(ctx, RM_E_INVALID, "reach must be finite and >= 0");
    if (n < 0 || n > std::numeric_limits<int32_t>::max()) return fail(ctx, RM_E_INVALID, "vertex count out of range");
    if (n > 0 && (!cells || !position)) return fail(ctx, RM_E_INVALID, "null cells or position");
    if (reinterpret_cast<uintptr_t>(cells) & 7) return fail(ctx, RM_E_INVALID, "cells must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(position) | reinterpret_cast<uintptr_t>(feature) | reinterpret_cast<uintptr_t>(count)) & 3)
        return fail(ctx, RM_E_INVALID, "position, feature and count must be 4-byte aligned");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU distance path");
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    return RM_OK;
}

// The parameter block and the query of rm_scene_sharpen: the active scene at the lattice's own time (fill_scene_query).  rho,
// half the longest body diagonal of a cell, and the limit reach * rho in the rule's order.
void fill_sharp(const rm_ctx *ctx, const rm_lattice *lat, const rm_sharp_query *q, RmRenderParams &p, RmSharpArgs &a) {
    fill_scene_query(ctx, lat->time, p);
    std::memset(&a, 0, sizeof a);
    a.lat = widen_lattice(*lat);
    const RmLattice &l = a.lat;
    double longest = 0.0;
    for (int s = 0; s < 4; ++s) {  // (du + dv) + dw, (du + dv) - dw, (du - dv) + dw, (du - dv) - dw
        double d[3];
        for (int c = 0; c < 3; ++c) {
            const double uv = s < 2 ? l.du[c] + l.dv[c] : l.du[c] - l.dv[c];
            d[c] = s % 2 == 0 ? uv + l.dw[c] : uv - l.dw[c];
        }
        const double length = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (s == 0 || length > longest) longest = length;
    }
    a.iso = q->iso;
    a.rank_tol = q->rank_tol;
    a.limit = q->reach * (0.5 * longest);
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
    a.nw = static_cast<unsigned int>(lat->nw);
    a.refine = q->refine;
}

// Both forms of rm_scene_field, rm_scene_points and rm_scene_sharpen, as ray_call is both forms of a ray query: the checks,
// the launch's two blocks, then staged_call with the entry's columns.  host: the buffers are the caller's host memory.

// The host form goes in chunks of whole lattice rows, at most 4 M points (16 B per point with every output: 64 MB); a row
// always fits (nu <= 65535).  The launch is told where its range starts.
int scene_field_call(rm_ctx *ctx, const rm_lattice *lattice, bool host, void *dist, void *dist32, void *count, void *stream) {
    if (!ctx) return RM_E_INVALID;
    int64_t n = 0;
    const int rc = check_field(ctx, lattice, dist, dist32, count, &n);
    if (rc || !n) return rc;
    RmRenderParams p;
    RmFieldArgs a;
    fill_field(ctx, lattice, p, a);
    if (const int erc = apply_exact(ctx, p)) return erc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const Column cols[] = {{dist, 8, &a.dist, false, true}, {dist32, 4, &a.dist32, false, true}, {count, 4, &a.count, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n, lattice->nu, kHostChunk, cols, 3, [&](int64_t first, int64_t m, hipStream_t s) {
        a.first = first;
        a.n = m;
        return (ctx->opt_length ? rm_launch_field_sqrt : rm_launch_field)(p, a, s, &ctx->last_kernel);
    });
}

// The host form goes in chunks of at most 4 M points, as the ray queries: 12 B per point go up, and the positions are written
// over the staged points (48 B per point with all six outputs: 192 MB).
int scene_points_call(rm_ctx *ctx, const rm_point_query *q, int64_t n, const void *points, bool host, void *position, void *dist, void *normal,
                      void *object, void *steps, void *count, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const int rc = check_points(ctx, q, n, static_cast<const float *>(points), host, position, dist, normal, object, steps, count);
    if (rc || !n) return rc;
    RmRenderParams p;
    RmPointArgs a;
    fill_points(ctx, q, p, a);
    if (const int erc = apply_exact(ctx, p)) return erc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const Column cols[] = {{points, 12, &a.points, true, false},  {position, 12, &a.position, false, true, 0}, {dist, 8, &a.dist, false, true},
                           {normal, 12, &a.normal, false, true}, {object, 4, &a.object, false, true},         {steps, 4, &a.steps, false, true},
                           {count, 4, &a.count, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n, 1, kHostChunk, cols, 7, [&](int64_t, int64_t m, hipStream_t s) {
        a.n = m;
        return (ctx->opt_length ? rm_launch_points_sqrt : rm_launch_points)(p, a, s, &ctx->last_kernel);
    });
}

// The host form goes in chunks of at most 4 M vertices: 8 B per vertex go up, 12 B and the optional outputs come back.
int scene_sharpen_call(rm_ctx *ctx, const rm_lattice *lattice, const rm_sharp_query *q, int64_t n, const void *cells, bool host, void *position,
                       void *feature, void *count, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const int rc = check_sharp(ctx, lattice, q, n, cells, position, feature, count);
    if (rc || !n) return rc;
    RmRenderParams p;
    RmSharpArgs a;
    fill_sharp(ctx, lattice, q, p, a);
    if (const int erc = apply_exact(ctx, p)) return erc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const Column cols[] = {{cells, 8, &a.cells, true, false}, {position, 12, &a.position, false, true}, {feature, 4, &a.feature, false, true},
                           {count, 4, &a.count, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n, 1, kHostChunk, cols, 4, [&](int64_t, int64_t m, hipStream_t s) {
        a.n = m;
        return (ctx->opt_length ? rm_launch_sharp_sqrt : rm_launch_sharp)(p, a, s, &ctx->last_kernel);
    });
}

// Both forms of the operations on rendered frames, in the same way: the checks, the kernel's argument block, then staged_call
// with the entry's columns -- in ONE trip (limit = n): a host form is one launch, as its device form.  The element of the four
// per-frame entries is a frame (n = n_frames; a column's bytes are its buffer's per frame), of rm_shade and rm_shade_field a
// pixel or a value.  host: the buffers are the caller's host memory.

// A frame set's pair absent on both sides, the image with RM_CMP_MAP_NONE and absent records are null columns.  Frames of
// several workgroups combine their partial records through the context's ring, taken ahead of the launch on the trip's stream.
int compare_call(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const rm_frame_set *a, const rm_frame_set *b, int32_t map, int32_t gain,
                 bool host, void *rgba, void *stats, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const int rc = check_compare(ctx, width, rows, n_frames, a, b, map, gain, rgba, stats);
    if (rc || n_frames == 0) return rc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npx = static_cast<size_t>(width) * static_cast<size_t>(rows), n = static_cast<size_t>(n_frames);
    if (npx == 0) {  // frames without a pixel: all-zero records, no image byte
        if (stats && host) std::memset(stats, 0, sizeof(rm_compare_stats) * n);
        else if (stats) RM_HIP(ctx, hipMemsetAsync(stats, 0, sizeof(rm_compare_stats) * n, static_cast<hipStream_t>(stream)));
        return RM_OK;
    }
    RmCompareArgs args;
    std::memset(&args, 0, sizeof args);
    args.npx = static_cast<int64_t>(npx);
    args.gain = static_cast<unsigned int>(map == RM_CMP_MAP_NONE ? 1 : gain);
    const int32_t per_frame = rm_compare_blocks_per_frame(args.npx, n_frames);
    const size_t entries = stats && per_frame > 1 ? static_cast<size_t>(per_frame) * n : 0;
    const Column cols[] = {{a->depth, npx, &args.depth_a, true, false},      {b->depth, npx, &args.depth_b, true, false},
                           {a->normal, 3 * npx, &args.normal_a, true, false}, {b->normal, 3 * npx, &args.normal_b, true, false},
                           {a->sdf, 2 * npx, &args.sdf_a, true, false},       {b->sdf, 2 * npx, &args.sdf_b, true, false},
                           {a->iters, 2 * npx, &args.iters_a, true, false},   {b->iters, 2 * npx, &args.iters_b, true, false},
                           {map == RM_CMP_MAP_NONE ? nullptr : rgba, 4 * npx, &args.rgba, false, true},
                           {stats, sizeof(rm_compare_stats), &args.stats, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n_frames, 1, n_frames, cols, 10, [&](int64_t, int64_t, hipStream_t s) {
        size_t first = 0;
        if (entries) {
            const hipError_t taken = ctx->compare.take(entries, &first);
            if (taken != hipSuccess) return taken;
            args.partials = ctx->compare.partials + first;
            args.counters = ctx->compare.counters + first;
        }
        const hipError_t e = rm_launch_compare(args, map, n_frames, per_frame, s, &ctx->last_kernel);
        if (entries) ctx->compare.launched(first, entries, s);  // (also behind a failed launch)
        return e;
    });
}

// Frames without a pixel still launch: one workgroup per frame writes the empty records, which carry the shift.  RM_HIST_ALL
// passes no normal buffer.  Frames of several workgroups add into scratch entries of the context's ring.
int hist_call(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const void *sdf, const void *iters, const void *normal, int32_t mask,
              int32_t bin_shift, int32_t lo_permille, int32_t hi_permille, bool host, void *hist, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const int rc = check_hist(ctx, width, rows, n_frames, sdf, iters, normal, mask, bin_shift, lo_permille, hi_permille, hist);
    if (rc || n_frames == 0) return rc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npx = static_cast<size_t>(width) * static_cast<size_t>(rows);
    RmHistArgs args;
    std::memset(&args, 0, sizeof args);
    args.npx = static_cast<int64_t>(npx);
    args.shift = static_cast<unsigned int>(bin_shift);
    args.lo_permille = static_cast<unsigned int>(lo_permille);
    args.hi_permille = static_cast<unsigned int>(hi_permille);
    args.want_surface = mask == RM_HIST_SURFACE;
    const int32_t per_frame = rm_compare_blocks_per_frame(args.npx, n_frames);
    const size_t entries = per_frame > 1 ? static_cast<size_t>(n_frames) : 0;
    const Column cols[] = {{sdf, 2 * npx, &args.sdf, true, false},
                           {iters, 2 * npx, &args.iters, true, false},
                           {mask == RM_HIST_ALL ? nullptr : normal, 3 * npx, &args.normal, true, false},
                           {hist, sizeof(rm_frame_hist), &args.hist, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n_frames, 1, n_frames, cols, 4, [&](int64_t, int64_t, hipStream_t s) {
        size_t first = 0;
        if (entries) {
            const hipError_t taken = ctx->hists.take(entries, &first);
            if (taken != hipSuccess) return taken;
            args.scratch = ctx->hists.entries + first;
        }
        const hipError_t e = rm_launch_hist(args, mask != RM_HIST_ALL, n_frames, per_frame, s, &ctx->last_kernel);
        if (entries) ctx->hists.launched(first, entries, s);  // (also behind a failed launch)
        return e;
    });
}

// Absent records are a null column: every frame then takes lo and hi.
int shade_ranged_call(rm_ctx *ctx, int32_t counter, int32_t width, int32_t rows, int32_t n_frames, const void *values, const void *hist, uint32_t lo,
                      uint32_t hi, bool host, void *rgba, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const int rc = check_shade_ranged(ctx, counter, width, rows, n_frames, values, hist, lo, hi, rgba);
    const size_t npx = static_cast<size_t>(width) * static_cast<size_t>(rows);
    if (rc || n_frames == 0 || npx == 0) return rc;
    RmShadeRangedArgs args;
    std::memset(&args, 0, sizeof args);
    args.npx = static_cast<int64_t>(npx);
    args.counter = static_cast<unsigned int>(counter);
    args.lo = lo;
    args.hi = hi;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const Column cols[] = {{values, 2 * npx, &args.values, true, false}, {hist, sizeof(rm_frame_hist), &args.hist, true, false},
                           {rgba, 4 * npx, &args.rgba, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n_frames, 1, n_frames, cols, 3, [&](int64_t, int64_t, hipStream_t s) {
        return rm_launch_shade_ranged(args, n_frames, s, &ctx->last_kernel);
    });
}

int shade_lit_call(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const void *depth, const void *normal, const void *lit, const void *ao,
                   bool host, void *rgba, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const int rc = check_shade_lit(ctx, width, rows, n_frames, depth, normal, lit, ao, rgba);
    const size_t npx = static_cast<size_t>(width) * static_cast<size_t>(rows);
    if (rc || n_frames == 0 || npx == 0) return rc;
    RmShadeLitArgs args;
    std::memset(&args, 0, sizeof args);
    args.npx = static_cast<int64_t>(npx);
    for (int k = 0; k < 3; ++k) args.light[k] = ctx->light[k];
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const Column cols[] = {{depth, npx, &args.depth, true, false}, {normal, 3 * npx, &args.normal, true, false}, {lit, 4 * npx, &args.lit, true, false},
                           {ao, 4 * npx, &args.ao, true, false},   {rgba, 4 * npx, &args.rgba, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n_frames, 1, n_frames, cols, 5, [&](int64_t, int64_t, hipStream_t s) {
        return rm_launch_shade_lit(args, n_frames, s, &ctx->last_kernel);
    });
}

// The device check comes first here, and the entry leaves rm_last_kernel alone.
int shade_call(rm_ctx *ctx, int32_t shader, int32_t width, int32_t height, const void *depth, const void *normal, const void *sdf, const void *iters,
               bool host, void *rgba, void *stream) {
    RM_NEED_DEVICE(ctx, "host-only context");
    if (width < 0 || height < 0) return fail(ctx, RM_E_INVALID, "negative size");
    if (!depth || !normal || !sdf || !iters || !rgba) return fail(ctx, RM_E_INVALID, "null buffer");
    const int64_t npx = static_cast<int64_t>(width) * height;
    if (!npx) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    struct {
        const uint8_t *depth, *normal;
        const uint16_t *sdf, *iters;
        uint8_t *rgba;
    } d;
    const Column cols[] = {{depth, 1, &d.depth, true, false}, {normal, 3, &d.normal, true, false}, {sdf, 2, &d.sdf, true, false},
                           {iters, 2, &d.iters, true, false}, {rgba, 4, &d.rgba, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), npx, 1, npx, cols, 5, [&](int64_t, int64_t m, hipStream_t s) {
        return rm_launch_shade(norm_shader(shader), m, d.depth, d.normal, d.sdf, d.iters, d.rgba, ctx->light, s);
    });
}

int shade_field_call(rm_ctx *ctx, const rm_field_shade *shade, int64_t n, const void *values, bool host, void *rgba, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const int rc = check_shade_field(ctx, shade, n, values, rgba);
    if (rc || !n) return rc;
    RmShadeFieldArgs args;
    std::memset(&args, 0, sizeof args);
    args.n = n;
    args.range = shade->range;
    args.band = shade->band;
    args.line = shade->line;
    args.lo = shade->lo;
    args.hi = shade->hi;
    args.map = shade->map;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const Column cols[] = {{values, shade->map == RM_FIELD_MAP_DISTANCE ? 8u : 4u, &args.values, true, false}, {rgba, 4, &args.rgba, false, true}};
    return staged_call(ctx, host, static_cast<hipStream_t>(stream), n, 1, n, cols, 2, [&](int64_t, int64_t, hipStream_t s) {
        return rm_launch_shade_field(args, s, &ctx->last_kernel);
    });
}


// What rm_scene_edit_spheres and rm_scene_edit_balls share: the checks of an edit list in their order -- the list, each edit
// without the scene, the scene, each index at its turn -- and the edits applied to the active scene's object list `d`.
// on_ball(centre, radius) takes every sphere version an edit removes (SET, REMOVE) or adds (SET, INSERT), in edit order.
template <typename OnBall>
int replay_sphere_edits(rm_ctx *ctx, const rm_sphere_edit *edits, int32_t n_edits, SceneDesc &d, OnBall on_ball) {
    if (n_edits < 0 || (n_edits > 0 && !edits)) return fail(ctx, RM_E_INVALID, "bad edit list");
    for (int32_t i = 0; i < n_edits; ++i) {  // what can be said of an edit without the scene
        const rm_sphere_edit &e = edits[i];
        if (e.op != RM_EDIT_SET && e.op != RM_EDIT_INSERT && e.op != RM_EDIT_REMOVE) return fail(ctx, RM_E_INVALID, "edit " + std::to_string(i) + ": unknown op");
        if (e.reserved != 0) return fail(ctx, RM_E_INVALID, "edit " + std::to_string(i) + ": reserved must be 0");
        if (e.op != RM_EDIT_REMOVE &&
            !(std::isfinite(e.center[0]) && std::isfinite(e.center[1]) && std::isfinite(e.center[2]) && std::isfinite(e.radius)))
            return fail(ctx, RM_E_INVALID, "edit " + std::to_string(i) + ": non-finite sphere centre or radius");
    }
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    // the active scene's object list
    if (ctx->scene_is_uploaded) {
        if (ctx->uploaded.kind != SceneDesc::kSpheres) return fail(ctx, RM_E_UNSUPPORTED, "the active scene is not a sphere list");
        d.centers = ctx->uploaded.centers;
        d.radii = ctx->uploaded.radii;
    } else if (!rmh::preset_spheres(ctx->scene_preset, d.centers, d.radii)) {
        return fail(ctx, RM_E_UNSUPPORTED, "the active scene is not a sphere list");
    }
    d.kind = SceneDesc::kSpheres;
    for (int32_t i = 0; i < n_edits; ++i) {
        const rm_sphere_edit &e = edits[i];
        const int64_t n = static_cast<int64_t>(d.radii.size());
        if (e.index < 0 || e.index > n || (e.op != RM_EDIT_INSERT && e.index == n))
            return fail(ctx, RM_E_INVALID, "edit " + std::to_string(i) + ": index out of range");
        const auto c = d.centers.begin() + 3 * static_cast<std::ptrdiff_t>(e.index);
        const auto r = d.radii.begin() + e.index;
        if (e.op != RM_EDIT_INSERT) on_ball(&*c, *r);
        if (e.op == RM_EDIT_REMOVE) {
            d.centers.erase(c, c + 3);
            d.radii.erase(r);
        } else if (e.op == RM_EDIT_INSERT) {
            d.centers.insert(c, e.center, e.center + 3);
            d.radii.insert(r, e.radius);
        } else {
            std::copy(e.center, e.center + 3, c);
            *r = e.radius;
        }
        if (e.op != RM_EDIT_REMOVE) on_ball(e.center, e.radius);
    }
    return RM_OK;
}
}  // namespace

extern "C" {

const char *rm_version(void) { return "cpu-raymarcher_amd 0.1 (gfx950)"; }

int rm_create(int device, rm_ctx **out) {
    if (!out) return RM_E_INVALID;
    *out = nullptr;
    rm_ctx *ctx = new (std::nothrow) rm_ctx();
    if (!ctx) return RM_E_NOMEM;
    rmh::phong_light_dir(ctx->light);
    ctx->hw_queues = read_hw_queues();  // once: what the variable says later is not what the runtime started with
    if (device >= 0) {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || device >= count) {
            delete ctx;
            return RM_E_NO_DEVICE;
        }
        e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamCreate(&ctx->stream);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&ctx->d_diag), sizeof(RmDiagDevice));
        if (e == hipSuccess) e = ctx->slots.init();
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&ctx->d_stamps), (40 + 3 * 8192 + 2048 * 48) * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(ctx->d_stamps, 0, (40 + 3 * 8192 + 2048 * 48) * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(ctx->d_stamps + 6, 0xFF, sizeof(unsigned long long));
        if (e != hipSuccess) {
            delete ctx;
            return RM_E_HIP;
        }
        ctx->device = device;
        ctx->has_device = true;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            ctx->num_cus = cus;
    }
    *out = ctx;
    return RM_OK;
}

void rm_destroy(rm_ctx *ctx) {
    if (!ctx) return;
    if (ctx->has_device) {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
        free_device_scene(ctx);
        (void)hipFree(ctx->scratch);
        if (ctx->scratch_busy) (void)hipEventDestroy(ctx->scratch_busy);
        (void)hipFree(ctx->d_diag);
        (void)hipFree(ctx->d_stamps);
        for (auto &t : ctx->tables) (void)hipFree(t.dev);
        ctx->slots.release();
        ctx->lpt.release();
        ctx->oct_tables.release();
        ctx->frames.release();
        ctx->compare.release();
        ctx->hists.release();
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

const char *rm_last_error(const rm_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
const char *rm_last_kernel(const rm_ctx *ctx) { return ctx && ctx->last_kernel ? ctx->last_kernel : ""; }

int rm_algorithm_from_string(const char *s) {
    if (!s) return RM_ALG_SPHERE_TRACER;
    if (!std::strcmp(s, "fixed-step")) return RM_ALG_FIXED_STEP;
    if (!std::strcmp(s, "adaptive-step")) return RM_ALG_ADAPTIVE_STEP;
    if (!std::strcmp(s, "adaptive-step-v2")) return RM_ALG_ADAPTIVE_STEP_V2;
    if (!std::strcmp(s, "adaptive-step-v3")) return RM_ALG_ADAPTIVE_STEP_V3;
    return RM_ALG_SPHERE_TRACER;  // 'sphere-tracer' and the default branch
}

int rm_accel_from_string(const char *s) {
    if (s && !std::strcmp(s, "Octree")) return RM_ACCEL_OCTREE;
    if (s && !std::strcmp(s, "BVH")) return RM_ACCEL_BVH;
    return RM_ACCEL_NONE;
}

int rm_shader_from_string(const char *s) {
    if (s && !std::strcmp(s, "phong")) return RM_SHADE_PHONG;
    if (s && !std::strcmp(s, "sdf-heatmap")) return RM_SHADE_SDF_HEATMAP;
    if (s && !std::strcmp(s, "iteration-heatmap")) return RM_SHADE_ITERATION_HEATMAP;
    return RM_SHADE_NORMAL;
}

int rm_preset_count(void) { return rmh::kPresetCount; }

int rm_scene_from_preset(rm_ctx *ctx, int32_t preset_index, int32_t accel) {
    if (!ctx) return RM_E_INVALID;
    if (preset_index == RM_SCENE_UPLOADED) return fail(ctx, RM_E_INVALID, "not a preset index");
    // force a rebuild only when something changed
    return ensure_scene(ctx, preset_index, accel);
}

int rm_scene_from_spheres(rm_ctx *ctx, const float *centers_xyz, const double *radii, int32_t n, int32_t accel) {
    if (!ctx) return RM_E_INVALID;
    if (n < 0 || (n > 0 && (!centers_xyz || !radii))) return fail(ctx, RM_E_INVALID, "bad sphere list");
    SceneDesc d;
    d.kind = SceneDesc::kSpheres;
    if (n) d.centers.assign(centers_xyz, centers_xyz + 3 * static_cast<size_t>(n));
    if (n) d.radii.assign(radii, radii + n);
    return set_uploaded_scene(ctx, std::move(d), accel);
}

int rm_scene_edit_balls(rm_ctx *ctx, const rm_sphere_edit *edits, int32_t n_edits, rm_ball *balls, int32_t cap, int32_t *n_balls) {
    if (!ctx) return RM_E_INVALID;
    if (!n_balls || cap < 0 || (cap > 0 && !balls)) return fail(ctx, RM_E_INVALID, "bad ball buffer");
    *n_balls = 0;
    SceneDesc d;
    int32_t n = 0;
    const int rc = replay_sphere_edits(ctx, edits, n_edits, d, [&](const float *centre, double radius) {
        if (n < cap) {
            rm_ball &b = balls[n];
            std::copy(centre, centre + 3, b.center);
            b.reserved = 0;
            b.radius = radius;
        }
        ++n;
    });
    if (rc) return rc;  // (balls written ahead of a refused index mean nothing)
    *n_balls = n;
    return RM_OK;
}

int rm_scene_edit_spheres(rm_ctx *ctx, const rm_sphere_edit *edits, int32_t n_edits) {
    if (!ctx) return RM_E_INVALID;
    SceneDesc d;
    if (const int bad = replay_sphere_edits(ctx, edits, n_edits, d, [](const float *, double) {})) return bad;
    if (n_edits == 0) return RM_OK;
    // from here on as rm_scene_from_spheres(edited list, same acceleration structure): nothing changes unless the build succeeds
    std::string kernel_name = ctx->last_kernel ? ctx->last_kernel : "";
    const rmh::PairLoops loops = (ctx->has_device && ctx->opt_device_build) ? device_pair_loops(ctx) : rmh::PairLoops();
    const int rc = set_scene(ctx, d, ctx->host.accel, true, RM_SCENE_UPLOADED, &loops);
    ctx->last_kernel_kept.swap(kernel_name);  // not a render entry: rm_last_kernel keeps its answer
    ctx->last_kernel = ctx->last_kernel_kept.c_str();
    if (rc) return rc;
    ctx->uploaded = std::move(d);
    ctx->have_uploaded = true;
    return RM_OK;
}

int rm_debug_scene_table(rm_ctx *ctx, const char *name, int32_t from_device, void *out, int64_t cap, int64_t *bytes) {
    if (!ctx) return RM_E_INVALID;
    if (!name || !bytes || cap < 0 || (cap > 0 && !out)) return fail(ctx, RM_E_INVALID, "bad arguments");
    *bytes = 0;
    const void *host = nullptr, *dev = nullptr;
    size_t size = 0;
    bool found = false;
#define RM_X(nm, always)                                                                        \
    if (!found && !std::strcmp(name, #nm)) {                                                    \
        found = true;                                                                           \
        host = ctx->host.nm.data();                                                             \
        size = ctx->host.nm.size() * sizeof(decltype(rmh::HostScene::nm)::value_type);          \
        dev = ctx->dev.nm;                                                                      \
    }
    RM_SCENE_ARRAYS(RM_X)
#undef RM_X
    if (!found) return fail(ctx, RM_E_INVALID, std::string("unknown scene table ") + name);
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    if (from_device && !ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: read the host copy");
    *bytes = static_cast<int64_t>(size);
    if (!size || static_cast<int64_t>(size) > cap) return RM_OK;
    if (!from_device) {
        std::memcpy(out, host, size);
        return RM_OK;
    }
    if (!dev) return fail(ctx, RM_E_HIP, std::string("no device copy of scene table ") + name);
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RM_HIP(ctx, hipDeviceSynchronize());
    RM_HIP(ctx, hipMemcpy(out, dev, size, hipMemcpyDeviceToHost));
    return RM_OK;
}

int rm_scene_from_nodes(rm_ctx *ctx, const rm_node *nodes, int32_t n_nodes, const int32_t *roots, int32_t n_roots,
                        int32_t accel) {
    if (!ctx) return RM_E_INVALID;
    if (n_nodes < 0 || n_roots < 0 || (n_nodes > 0 && !nodes) || (n_roots > 0 && !roots))
        return fail(ctx, RM_E_INVALID, "bad node list");
    SceneDesc d;
    d.kind = SceneDesc::kNodes;
    d.nodes.resize(static_cast<size_t>(n_nodes));
    for (int i = 0; i < n_nodes; ++i) {
        d.nodes[i].type = nodes[i].type;
        d.nodes[i].a = nodes[i].child_a;
        d.nodes[i].b = nodes[i].child_b;
        std::memcpy(d.nodes[i].m, nodes[i].world_to_local, sizeof d.nodes[i].m);
        for (int k = 0; k < 6; ++k) d.nodes[i].params[k] = nodes[i].params[k];
    }
    if (n_roots) d.roots.assign(roots, roots + n_roots);
    return set_uploaded_scene(ctx, std::move(d), accel);
}

int rm_scale_transform(float *m, double x, double y, double z) {
    if (!m || !std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return RM_E_INVALID;
    rmh::scale_transform(m, x, y, z);
    return RM_OK;
}

int rm_scene_set_time(rm_ctx *ctx, double time) {
    if (!ctx) return RM_E_INVALID;
    if (!std::isfinite(time)) return fail(ctx, RM_E_INVALID, "non-finite time");
    ctx->time = time;
    return RM_OK;
}

int rm_scene_from_prims(rm_ctx *ctx, const rm_prim *prims, int32_t n, int32_t accel) {
    if (!ctx) return RM_E_INVALID;
    if (n < 0 || (n > 0 && !prims)) return fail(ctx, RM_E_INVALID, "bad primitive list");
    SceneDesc d;
    d.kind = SceneDesc::kPrims;
    d.prims.resize(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        d.prims[i].type = prims[i].type;
        std::memcpy(d.prims[i].m, prims[i].world_to_local, sizeof d.prims[i].m);
        for (int k = 0; k < 3; ++k) d.prims[i].params[k] = prims[i].params[k];
    }
    return set_uploaded_scene(ctx, std::move(d), accel);
}

int rm_make_transform(double x, double y, double z, const float *rotation_xyz, float *world_to_local16) {
    if (!world_to_local16 || !std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return RM_E_INVALID;
    if (rotation_xyz)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(rotation_xyz[k])) return RM_E_INVALID;
    rmh::make_transform(x, y, z, rotation_xyz, world_to_local16);
    return RM_OK;
}

int rm_scene_get_info(const rm_ctx *ctx, rm_scene_info *out) {
    if (!ctx || !out) return RM_E_INVALID;
    if (!ctx->have_scene) return RM_E_NO_SCENE;
    std::memset(out, 0, sizeof *out);
    const rmh::HostScene &h = ctx->host;
    out->n_prims = scene_n_prims(ctx);
    out->accel = h.accel;
    out->preset_index = ctx->scene_preset;
    out->bvh_nodes = static_cast<int32_t>(h.bvh.size());
    out->bvh_leaves = h.bvh_leaves;
    out->bvh_depth = h.bvh_depth;
    out->oct_nodes = static_cast<int32_t>(h.oct.size());
    out->oct_leaves = h.oct_leaves;
    out->oct_empty_leaves = h.oct_empty;
    out->oct_max_leaf_prims = h.oct_max_leaf;
    std::memcpy(out->root_min, h.root_min, sizeof h.root_min);
    std::memcpy(out->root_max, h.root_max, sizeof h.root_max);
    out->nodes_in_lds = static_cast<int32_t>(ctx->opt_lds);
    if (h.program) out->program = h.prog_slots | (h.prog_vals << 8) | (static_cast<int32_t>(h.prog.size()) << 16);
    return RM_OK;
}

int rm_camera_from_angles(double pitch, double yaw, float *rot9, float *origin3) {
    if (!rot9 || !origin3 || !std::isfinite(pitch) || !std::isfinite(yaw)) return RM_E_INVALID;
    rmh::camera_from_angles(pitch, yaw, rot9, origin3);
    return RM_OK;
}

int rm_render_tile_device(rm_ctx *ctx, const rm_job *job, int32_t shader, void *d_depth, void *d_normal, void *d_sdf,
                          void *d_iters, void *d_rgba, void *stream) {
    return render_device(ctx, job, shader, Stripes(), {d_depth, d_normal, d_sdf, d_iters, d_rgba}, stream);
}

int rm_render_frames_device(rm_ctx *ctx, const rm_job *job, int32_t shader, const rm_view *views, int32_t n_views, void *d_depth,
                            void *d_normal, void *d_sdf, void *d_iters, void *d_rgba, void *d_acc, void *stream) {
    if (!ctx) return RM_E_INVALID;
    if (!job) return fail(ctx, RM_E_INVALID, "null job");
    if (n_views < 0 || n_views > 65535) return fail(ctx, RM_E_INVALID, "n_views must be in [0, 65535] (one grid dimension)");
    if (n_views > 0 && !views) return fail(ctx, RM_E_INVALID, "null views");
    for (int32_t k = 0; k < n_views; ++k)
        if (!std::isfinite(views[k].camera_pitch) || !std::isfinite(views[k].camera_yaw) || !std::isfinite(views[k].time))
            return fail(ctx, RM_E_INVALID, "non-finite angle or time in view " + std::to_string(k));
    if (d_acc && (reinterpret_cast<uintptr_t>(d_acc) & 7)) return fail(ctx, RM_E_INVALID, "the accumulators must be 8-byte aligned");
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context: there is no CPU render path");
    // everything the frames share, defaulted and clamped as for rm_render_tile_device; the job's own camera and time are not read
    rm_job shared = *job;
    shared.camera_pitch = shared.camera_yaw = shared.time = 0.0;
    const double scene_time = ctx->time;
    RmRenderParams p;
    const int rc = fill_params(ctx, &shared, p);
    ctx->time = scene_time;  // (fill_params stores the job's time there; this entry leaves rm_scene_set_time's value alone)
    if (rc) return rc;
    if (n_views == 0) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    p.variant = 1;  // the ahead-of-time one-ray-per-lane kernels, 8 x 8 wave tiles unless tile_w was set (fill_params)
    if (!ctx->tile_w_set) p.tile_w = 8;
    p.shader = norm_shader(shader);
    p.depth = static_cast<uint8_t *>(d_depth);
    p.normal = static_cast<uint8_t *>(d_normal);
    p.sdf = static_cast<uint16_t *>(d_sdf);
    p.iters = static_cast<uint16_t *>(d_iters);
    p.rgba = static_cast<uint8_t *>(d_rgba);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const bool empty = p.local_rows <= 0 || p.width <= 0;
    const RmFrameView *d_views = nullptr;
    RmFrameDiagBlock *blocks = nullptr;
    size_t first = 0;
    if (!empty) {
        RM_HIP(ctx, ctx->frames.take(static_cast<size_t>(n_views), &first));
        RmFrameView *h = ctx->frames.host + first;
        for (int32_t k = 0; k < n_views; ++k) {
            rmh::camera_from_angles(views[k].camera_pitch, views[k].camera_yaw, h[k].rot, h[k].origin);
            for (int a = 0; a < 3; ++a) h[k].origin_d[a] = h[k].origin[a];
            h[k].time = views[k].time;
        }
        d_views = ctx->frames.dev + first;
        blocks = d_acc ? ctx->frames.blocks + first : nullptr;
    }
    hipError_t e = empty ? hipSuccess
                         : hipMemcpyAsync(ctx->frames.dev + first, ctx->frames.host + first, static_cast<size_t>(n_views) * sizeof(RmFrameView),
                                          hipMemcpyHostToDevice, hs);
    if (e == hipSuccess)
        e = (ctx->opt_length ? rm_launch_frames_sqrt : rm_launch_frames)(p, d_views, n_views, blocks, static_cast<RmDiagDevice *>(d_acc), hs,
                                                                         &ctx->last_kernel);
    if (!empty) ctx->frames.launched(first, static_cast<size_t>(n_views), hs);  // (also behind a failed attempt: the copy may be queued)
    if (e != hipSuccess) return hip_fail(ctx, e, "rm_render_frames_device");
    return RM_OK;
}

int rm_compare_frames_device(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const rm_frame_set *a, const rm_frame_set *b,
                             int32_t map, int32_t gain, void *d_rgba, void *d_stats, void *stream) {
    return compare_call(ctx, width, rows, n_frames, a, b, map, gain, false, d_rgba, d_stats, stream);
}

int rm_compare_frames(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const rm_frame_set *a, const rm_frame_set *b, int32_t map,
                      int32_t gain, uint8_t *rgba, rm_compare_stats *stats) {
    return compare_call(ctx, width, rows, n_frames, a, b, map, gain, true, rgba, stats, nullptr);
}

int rm_counter_hist_device(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const void *d_sdf, const void *d_iters,
                           const void *d_normal, int32_t mask, int32_t bin_shift, int32_t lo_permille, int32_t hi_permille, void *d_hist,
                           void *stream) {
    return hist_call(ctx, width, rows, n_frames, d_sdf, d_iters, d_normal, mask, bin_shift, lo_permille, hi_permille, false, d_hist, stream);
}

int rm_counter_hist(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const uint16_t *sdf, const uint16_t *iters,
                    const uint8_t *normal, int32_t mask, int32_t bin_shift, int32_t lo_permille, int32_t hi_permille, rm_frame_hist *hist) {
    return hist_call(ctx, width, rows, n_frames, sdf, iters, normal, mask, bin_shift, lo_permille, hi_permille, true, hist, nullptr);
}

int rm_shade_ranged_device(rm_ctx *ctx, int32_t counter, int32_t width, int32_t rows, int32_t n_frames, const void *d_counter,
                           const void *d_hist, uint32_t lo, uint32_t hi, void *d_rgba, void *stream) {
    return shade_ranged_call(ctx, counter, width, rows, n_frames, d_counter, d_hist, lo, hi, false, d_rgba, stream);
}

int rm_shade_ranged(rm_ctx *ctx, int32_t counter, int32_t width, int32_t rows, int32_t n_frames, const uint16_t *values,
                    const rm_frame_hist *hist, uint32_t lo, uint32_t hi, uint8_t *rgba) {
    return shade_ranged_call(ctx, counter, width, rows, n_frames, values, hist, lo, hi, true, rgba, nullptr);
}

int rm_shade_lit_device(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const void *d_depth, const void *d_normal, const void *d_lit,
                        const void *d_ao, void *d_rgba, void *stream) {
    return shade_lit_call(ctx, width, rows, n_frames, d_depth, d_normal, d_lit, d_ao, false, d_rgba, stream);
}

int rm_shade_lit(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const uint8_t *depth, const uint8_t *normal, const float *lit,
                 const float *ao, uint8_t *rgba) {
    return shade_lit_call(ctx, width, rows, n_frames, depth, normal, lit, ao, true, rgba, nullptr);
}

int rm_sweep_views(double pitch, double yaw, double d_pitch, double d_yaw, double time0, double d_time, int32_t n, rm_view *views) {
    if (!std::isfinite(pitch) || !std::isfinite(yaw) || !std::isfinite(d_pitch) || !std::isfinite(d_yaw) || !std::isfinite(time0) ||
        !std::isfinite(d_time) || n < 0 || (n > 0 && !views))
        return RM_E_INVALID;
    double p = rmh::clamp_pitch(pitch), y = yaw;  // Camera.setAngles (camera.ts:58-62)
    for (int32_t k = 0; k < n; ++k) {
        if (k) {  // Camera.rotateCamera (camera.ts:26-31)
            p = rmh::clamp_pitch(p + d_pitch);
            y += d_yaw;
        }
        views[k].camera_pitch = p;
        views[k].camera_yaw = y;
        views[k].time = time0 + static_cast<double>(k) * d_time;
    }
    return RM_OK;
}

int rm_render_attach_diagnostics(rm_ctx *ctx, void *d_acc) {
    RM_NEED_DEVICE(ctx, "host-only context");
    if (d_acc && (reinterpret_cast<uintptr_t>(d_acc) & 7)) return fail(ctx, RM_E_INVALID, "the accumulator must be 8-byte aligned");
    ctx->diag_next = d_acc;
    return RM_OK;
}

int rm_stripe_rows(int32_t y_start, int32_t y_end, int32_t stripe_rows, int32_t n_parts, int32_t part) {
    if (stripe_rows <= 0 || n_parts <= 0 || part < 0 || part >= n_parts) return RM_E_INVALID;
    const int64_t rows = y_end > y_start ? static_cast<int64_t>(y_end) - y_start : 0;
    int64_t mine = 0;
    for (int64_t s = part; s * stripe_rows < rows; s += n_parts) {
        const int64_t a = s * stripe_rows, b = a + stripe_rows;
        mine += (b < rows ? b : rows) - a;
    }
    return static_cast<int>(mine);
}

int rm_render_stripes_device(rm_ctx *ctx, const rm_job *job, int32_t shader, int32_t stripe_rows, int32_t n_parts,
                             int32_t part, void *d_depth, void *d_normal, void *d_sdf, void *d_iters, void *d_rgba,
                             void *stream) {
    Stripes s;
    s.kind = Stripes::kPart;
    s.stripe_rows = stripe_rows;
    s.n_parts = n_parts;
    s.part = part;
    return render_device(ctx, job, shader, s, {d_depth, d_normal, d_sdf, d_iters, d_rgba}, stream);
}

int rm_deal_stripes(int32_t rows, int32_t stripe_rows, int32_t n_parts, const int32_t *weights, int32_t *owner) {
    if (rows < 0 || stripe_rows <= 0 || n_parts <= 0 || n_parts > 65535 || !owner) return RM_E_INVALID;
    int64_t total = 0;
    for (int p = 0; p < n_parts; ++p) {
        const int64_t w = weights ? weights[p] : 1;
        if (w <= 0 || w > (1 << 20)) return RM_E_INVALID;
        total += w;
    }
    const int n = static_cast<int>((static_cast<int64_t>(rows) + stripe_rows - 1) / stripe_rows);
    // smooth weighted round-robin: credit every part its weight, hand the stripe to the richest (lowest index on a
    // tie), charge it the total.  Equal weights: 0, 1, ..., n_parts - 1, 0, 1, ...
    std::vector<int64_t> credit(static_cast<size_t>(n_parts), 0);
    for (int s = 0; s < n; ++s) {
        int best = 0;
        for (int p = 0; p < n_parts; ++p) {
            credit[p] += weights ? weights[p] : 1;
            if (credit[p] > credit[best]) best = p;
        }
        credit[best] -= total;
        owner[s] = best;
    }
    return n;
}

int rm_render_stripe_list_device(rm_ctx *ctx, const rm_job *job, int32_t shader, int32_t stripe_rows, const int32_t *stripe_ids,
                                 int32_t n_stripes, void *d_depth, void *d_normal, void *d_sdf, void *d_iters, void *d_rgba,
                                 void *stream) {
    Stripes s;
    s.kind = Stripes::kList;
    s.stripe_rows = stripe_rows;
    s.ids = stripe_ids;
    s.n_ids = n_stripes;
    return render_device(ctx, job, shader, s, {d_depth, d_normal, d_sdf, d_iters, d_rgba}, stream);
}

int rm_assemble_frame_device(rm_ctx *ctx, const void *d_gathered, int64_t rank_stride, int64_t section_offset, int32_t row_bytes,
                             int32_t height, int32_t stripe_rows, const int32_t *owner, int32_t n_stripes, int32_t world,
                             void *d_frame, int64_t acc_offset, void *d_acc, void *stream) {
    RM_NEED_DEVICE(ctx, "host-only context");
    if (!d_gathered || !d_frame || !owner) return fail(ctx, RM_E_INVALID, "null buffer");
    if (row_bytes <= 0 || height < 0 || stripe_rows <= 0 || world <= 0 || world > 65535 || rank_stride < 0 || section_offset < 0)
        return fail(ctx, RM_E_INVALID, "bad frame geometry");
    if (n_stripes != (height + stripe_rows - 1) / stripe_rows || n_stripes > 65535)
        return fail(ctx, RM_E_INVALID, "owner[] must name every stripe of the frame (at most 65535)");
    if (acc_offset >= 0 && (acc_offset % 8 != 0 || rank_stride % 8 != 0)) return fail(ctx, RM_E_INVALID, "accumulators must be 8-byte aligned");
    // frame stripe s -> (rank, position among that rank's stripes): the rank packed its stripes in increasing y
    std::vector<int32_t> src(static_cast<size_t>(n_stripes));
    std::vector<int32_t> seen(static_cast<size_t>(world), 0);
    for (int s = 0; s < n_stripes; ++s) {
        if (owner[s] < 0 || owner[s] >= world) return fail(ctx, RM_E_INVALID, "owner out of range");
        src[s] = (owner[s] << 16) | seen[owner[s]]++;
    }
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const int32_t *d_src = nullptr;
    int rc = device_table(ctx, src.data(), src.size(), &d_src);
    if (rc) return rc;
    RM_HIP(ctx, rm_launch_assemble(static_cast<const unsigned char *>(d_gathered), rank_stride, section_offset, row_bytes, height,
                                   stripe_rows, d_src, n_stripes, static_cast<unsigned char *>(d_frame), acc_offset, world,
                                   static_cast<RmDiagDevice *>(d_acc), static_cast<hipStream_t>(stream)));
    return RM_OK;
}

int rm_render_tile(rm_ctx *ctx, const rm_job *job, uint8_t *depth, uint8_t *normal, uint16_t *sdf, uint16_t *iters) {
    RM_NEED_DEVICE(ctx, "host-only context: there is no CPU render path");
    if (!job) return fail(ctx, RM_E_INVALID, "null job");
    if (!depth || !normal || !sdf || !iters) return fail(ctx, RM_E_INVALID, "null output buffer");
    const int64_t rows = job->y_end > job->y_start ? static_cast<int64_t>(job->y_end) - job->y_start : 0;
    const size_t npx = static_cast<size_t>(rows) * static_cast<size_t>(job->width > 0 ? job->width : 0);
    RM_HIP(ctx, hipSetDevice(ctx->device));
    Staging st{ctx};
    const size_t o_depth = st.region(npx), o_normal = st.region(3 * npx), o_sdf = st.region(2 * npx), o_iters = st.region(2 * npx);
    int rc = st.reserve();
    if (rc) return rc;
    rc = rm_render_tile_device(ctx, job, RM_SHADE_NORMAL, st.at<void>(o_depth), st.at<void>(o_normal), st.at<void>(o_sdf), st.at<void>(o_iters), nullptr,
                               ctx->stream);
    if (rc) return rc;
    if (npx) {
        RM_HIP(ctx, st.out(depth, o_depth, npx));
        RM_HIP(ctx, st.out(normal, o_normal, 3 * npx));
        RM_HIP(ctx, st.out(sdf, o_sdf, 2 * npx));
        RM_HIP(ctx, st.out(iters, o_iters, 2 * npx));
    }
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

int rm_shade_device(rm_ctx *ctx, int32_t shader, int32_t width, int32_t height, const void *d_depth,
                    const void *d_normal, const void *d_sdf, const void *d_iters, void *d_rgba, void *stream) {
    return shade_call(ctx, shader, width, height, d_depth, d_normal, d_sdf, d_iters, false, d_rgba, stream);
}

int rm_shade(rm_ctx *ctx, int32_t shader, int32_t width, int32_t height, const uint8_t *depth, const uint8_t *normal,
             const uint16_t *sdf, const uint16_t *iters, uint8_t *rgba) {
    return shade_call(ctx, shader, width, height, depth, normal, sdf, iters, true, rgba, nullptr);
}

int rm_reduce_counters_enqueue(rm_ctx *ctx, const void *d_sdf, const void *d_iters, int64_t n, void *d_acc,
                               void *stream) {
    if (!d_acc) return RM_E_INVALID;
    RM_NEED_DEVICE(ctx, "host-only context");
    if (n < 0 || (n > 0 && (!d_sdf || !d_iters))) return fail(ctx, RM_E_INVALID, "bad buffers");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    RM_HIP(ctx, rm_launch_reduce_init(static_cast<RmDiagDevice *>(d_acc), st));
    RM_HIP(ctx, rm_launch_reduce(static_cast<const uint16_t *>(d_sdf), static_cast<const uint16_t *>(d_iters), n,
                                 static_cast<RmDiagDevice *>(d_acc), st));
    return RM_OK;
}

int rm_reduce_counters_device(rm_ctx *ctx, const void *d_sdf, const void *d_iters, int64_t n, rm_diagnostics *out,
                              void *stream) {
    if (!out) return RM_E_INVALID;
    RM_NEED_DEVICE(ctx, "host-only context");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc0 = rm_reduce_counters_enqueue(ctx, d_sdf, d_iters, n, ctx->d_diag, stream);
    if (rc0) return rc0;
    RmDiagDevice res;
    RM_HIP(ctx, hipMemcpyAsync(&res, ctx->d_diag, sizeof res, hipMemcpyDeviceToHost, st));
    RM_HIP(ctx, hipStreamSynchronize(st));
    out->total_sdf_calls = res.total_sdf;
    out->total_iterations = res.total_iters;
    out->max_sdf_calls = res.max_sdf;
    out->min_sdf_calls = res.min_sdf;
    out->total_pixels = static_cast<uint64_t>(n);
    return RM_OK;
}

int rm_reduce_counters(rm_ctx *ctx, const uint16_t *sdf, const uint16_t *iters, int64_t n, rm_diagnostics *out) {
    if (!out) return RM_E_INVALID;
    RM_NEED_DEVICE(ctx, "host-only context");
    if (n < 0 || (n > 0 && (!sdf || !iters))) return fail(ctx, RM_E_INVALID, "bad buffers");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = 2 * static_cast<size_t>(n);
    Staging st{ctx};
    const size_t o_sdf = st.region(bytes), o_iters = st.region(bytes);
    int rc = st.reserve();
    if (rc) return rc;
    if (n) {
        RM_HIP(ctx, st.in(o_sdf, sdf, bytes));
        RM_HIP(ctx, st.in(o_iters, iters, bytes));
    }
    return rm_reduce_counters_device(ctx, st.at<void>(o_sdf), st.at<void>(o_iters), n, out, ctx->stream);  // (synchronises)
}

int rm_partition_rows(int32_t height, int32_t n_workers, int32_t i, int32_t *y_start, int32_t *y_end) {
    if (!y_start || !y_end || n_workers <= 0 || height < 0 || i < 0) return RM_E_INVALID;
    // main.ts:444-449
    const int64_t rows = (static_cast<int64_t>(height) + n_workers - 1) / n_workers;
    const int64_t a = static_cast<int64_t>(i) * rows, b = (static_cast<int64_t>(i) + 1) * rows;
    *y_start = static_cast<int32_t>(a < height ? a : height);
    *y_end = static_cast<int32_t>(b < height ? b : height);
    return RM_OK;
}

int rm_scene_distance(rm_ctx *ctx, const float *points_xyz, int64_t n, double *dist, uint32_t *count) {
    return points_call(ctx, points_xyz, n, dist, count, [] { return RM_OK; }, [&](const float *d_points, double *d_dist, uint32_t *d_count) {
        RmRenderParams p;
        fill_scene_query(ctx, ctx->time, p);
        const rmrtc::Kernel *special = specialised_kernel(ctx, p.accel, false);
        p.rtc_function = special ? special->distance : nullptr;
        return (ctx->opt_length ? rm_launch_distance_sqrt : rm_launch_distance)(p, d_points, n, d_dist, d_count, ctx->stream);
    });
}

int rm_lattice_points(const rm_lattice *lattice, int64_t first, int64_t n, float *points_xyz) {
    int64_t total = 0;
    if (lattice_error(lattice, &total)) return RM_E_INVALID;
    if (first < 0 || n < 0 || first > total || n > total - first || (n > 0 && !points_xyz)) return RM_E_INVALID;
    if (!n) return RM_OK;
    const int64_t nu = lattice->nu, nv = lattice->nv;
    int64_t row = first / nu, i = first % nu, k = row / nv, j = row % nv;
    for (int64_t at = 0; at < n; ++at) {
        for (int c = 0; c < 3; ++c) points_xyz[3 * at + c] = lattice_component(*lattice, c, i, j, k);
        if (++i == nu) {
            i = 0;
            if (++j == nv) {
                j = 0;
                ++k;
            }
        }
    }
    return RM_OK;
}

int rm_scene_field_device(rm_ctx *ctx, const rm_lattice *lattice, void *d_dist, void *d_dist32, void *d_count, void *stream) {
    return scene_field_call(ctx, lattice, false, d_dist, d_dist32, d_count, stream);
}

int rm_scene_field(rm_ctx *ctx, const rm_lattice *lattice, double *dist, float *dist32, uint32_t *count) {
    return scene_field_call(ctx, lattice, true, dist, dist32, count, nullptr);
}

int rm_scene_points_device(rm_ctx *ctx, const rm_point_query *q, int64_t n, const void *d_points, void *d_position, void *d_dist, void *d_normal,
                           void *d_object, void *d_steps, void *d_count, void *stream) {
    return scene_points_call(ctx, q, n, d_points, false, d_position, d_dist, d_normal, d_object, d_steps, d_count, stream);
}

int rm_scene_points(rm_ctx *ctx, const rm_point_query *q, int64_t n, const float *points_xyz, float *position, double *dist, float *normal,
                    int32_t *object, int32_t *steps, uint32_t *count) {
    return scene_points_call(ctx, q, n, points_xyz, true, position, dist, normal, object, steps, count, nullptr);
}

int rm_shade_field_device(rm_ctx *ctx, const rm_field_shade *shade, int64_t n, const void *d_values, void *d_rgba, void *stream) {
    return shade_field_call(ctx, shade, n, d_values, false, d_rgba, stream);
}

int rm_shade_field(rm_ctx *ctx, const rm_field_shade *shade, int64_t n, const void *values, uint8_t *rgba) {
    return shade_field_call(ctx, shade, n, values, true, rgba, nullptr);
}

int rm_mesh_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso, void *d_vertices,
                         int64_t cap_vertices, void *d_quads, int64_t cap_quads, void *d_info, void *stream) {
    if (!ctx) return RM_E_INVALID;
    const MeshCall m{lattice, true, d_values, value_type, iso, {d_vertices, d_quads, nullptr, nullptr, d_info, cap_vertices, cap_quads}};
    int64_t n = 0;
    bool cells = false;
    if (const int rc = check_mesh(ctx, m, &n, &cells)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // no cell, no launch: the totals are zero; else the map and the block totals
    return scratch_call(ctx, s, cells, d_info, sizeof(rm_mesh_info), {4 * static_cast<size_t>(n), 12 * mesh_blocks(n)},
                        [&](const Staging &st, const size_t *o) { return launch_mesh(ctx, st, m, n, o[0], o[1], s); });
}

int rm_scene_mesh(rm_ctx *ctx, const rm_lattice *lattice, double iso, float *vertices, int64_t cap_vertices, uint32_t *quads,
                  int64_t cap_quads, rm_mesh_info *info) {
    if (!ctx) return RM_E_INVALID;
    const MeshCall m{lattice, false, nullptr, RM_MESH_F64, iso, {vertices, quads, nullptr, nullptr, info, cap_vertices, cap_quads}};
    int64_t n = 0;
    bool cells = false;
    int rc = check_mesh(ctx, m, &n, &cells);
    if (rc) return rc;
    std::memset(info, 0, sizeof *info);
    if (!cells) return RM_OK;
    // The volume, the mesher's scratch and the outputs side by side in the scratch buffer; the lattice yields a vertex per cell
    // and three quads per point at most.
    const int64_t n_cells = static_cast<int64_t>(lattice->nu - 1) * (lattice->nv - 1) * (lattice->nw - 1);
    RM_HIP(ctx, hipSetDevice(ctx->device));
    Staging st{ctx};
    const size_t o_vol = st.region(8 * static_cast<size_t>(n)), o_map = st.region(4 * static_cast<size_t>(n)), o_totals = st.region(12 * mesh_blocks(n));
    const MeshRegions r(st, m.out, n_cells, 3 * n);
    if ((rc = st.reserve())) return rc;
    RmRenderParams p;
    RmFieldArgs a;
    fill_field(ctx, lattice, p, a);  // the field entries' own launch, at the lattice's time
    if (const int erc = apply_exact(ctx, p)) return erc;
    a.dist = st.at<double>(o_vol);
    a.first = 0;
    a.n = n;
    RM_HIP(ctx, (ctx->opt_length ? rm_launch_field_sqrt : rm_launch_field)(p, a, ctx->stream, &ctx->last_kernel));
    const MeshCall on_device{lattice, true, st.at<void>(o_vol), RM_MESH_F64, iso, r.on_device(st, m.out)};
    if ((rc = launch_mesh(ctx, st, on_device, n, o_map, o_totals, ctx->stream))) return rc;
    return read_mesh(ctx, st, r, m.out);
}

int rm_mesh_cells_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso, void *d_cells,
                         int64_t cap_vertices, void *d_info, void *stream) {
    if (!ctx) return RM_E_INVALID;
    if (reinterpret_cast<uintptr_t>(d_cells) & 7) return fail(ctx, RM_E_INVALID, "cells must be 8-byte aligned");
    MeshCall m{lattice, true, d_values, value_type, iso, {d_cells, nullptr, nullptr, nullptr, d_info, cap_vertices, 0}};  // checked as the vertices are
    int64_t n = 0;
    bool cells = false;
    if (const int rc = check_mesh(ctx, m, &n, &cells)) return rc;
    m.out.vertices = nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // no cell, no launch: the totals are zero; else the block totals (no map: nothing reads one)
    return scratch_call(ctx, s, cells, d_info, sizeof(rm_mesh_info), {12 * mesh_blocks(n)}, [&](const Staging &st, const size_t *o) -> int {
        RM_HIP(ctx, rm_launch_mesh_cells(mesh_args(st, m, n, o[0], o[0]), static_cast<long long *>(d_cells), s, &ctx->last_kernel));
        return RM_OK;
    });
}

int rm_scene_sharpen_device(rm_ctx *ctx, const rm_lattice *lattice, const rm_sharp_query *q, int64_t n, const void *d_cells, void *d_position,
                            void *d_feature, void *d_count, void *stream) {
    return scene_sharpen_call(ctx, lattice, q, n, d_cells, false, d_position, d_feature, d_count, stream);
}

int rm_scene_sharpen(rm_ctx *ctx, const rm_lattice *lattice, const rm_sharp_query *q, int64_t n, const int64_t *cells, float *position,
                     int32_t *feature, uint32_t *count) {
    return scene_sharpen_call(ctx, lattice, q, n, cells, true, position, feature, count, nullptr);
}

int rm_lattice_blocks(const rm_lattice *lattice, int32_t dims[3]) {
    SparseGrid g;
    if (!dims || sparse_error(lattice, &g, false)) return RM_E_INVALID;
    for (int c = 0; c < 3; ++c) dims[c] = g.nb[c];
    return RM_OK;
}

int rm_scene_blocks_device(rm_ctx *ctx, const rm_lattice *lattice, double iso, double lipschitz, void *d_slot, void *d_list, void *d_dist, void *d_info,
                           void *stream) {
    if (!ctx) return RM_E_INVALID;
    SparseGrid g;
    if (const char *bad = sparse_error(lattice, &g)) return fail(ctx, RM_E_INVALID, bad);
    if (!std::isfinite(iso)) return fail(ctx, RM_E_INVALID, "non-finite iso");
    if (!std::isfinite(lipschitz) || !(lipschitz > 0.0)) return fail(ctx, RM_E_INVALID, "lipschitz must be finite and > 0");
    if (!d_info) return fail(ctx, RM_E_INVALID, "null info");
    if (g.n_blocks > 0 && (!d_slot || !d_list)) return fail(ctx, RM_E_INVALID, "null slot or list");
    if (misaligned(d_slot, 3) || misaligned(d_list, 3)) return fail(ctx, RM_E_INVALID, "slot and list must be 4-byte aligned");
    if (misaligned(d_dist, 7) || misaligned(d_info, 7)) return fail(ctx, RM_E_INVALID, "dist and info must be 8-byte aligned");
    if (const int rc = need_device(ctx, "mesher", true)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // no block, no launch; else the scan's totals
    return scratch_call(ctx, s, g.n_blocks > 0, d_info, sizeof(rm_sparse_info), {4 * sparse_groups(g.n_blocks)}, [&](const Staging &st, const size_t *o) {
        return launch_blocks(ctx, lattice, g, iso, lipschitz, d_slot, d_list, d_dist, d_info, st.at<uint32_t>(o[0]), s);
    });
}

int rm_scene_tiles_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_list, int64_t n_kept, void *d_tiles, void *stream) {
    if (!ctx) return RM_E_INVALID;
    SparseGrid g;
    if (const char *bad = sparse_error(lattice, &g)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = kept_range_error(g, n_kept)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = kept_buffers_error(n_kept, d_list, d_tiles)) return fail(ctx, RM_E_INVALID, bad);
    if (misaligned(d_list, 3) || misaligned(d_tiles, 7)) return fail(ctx, RM_E_INVALID, "list must be 4-byte and tiles 8-byte aligned");
    if (const int rc = need_device(ctx, "distance path", true)) return rc;
    if (!n_kept) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_tiles(ctx, lattice, g, d_list, n_kept, d_tiles, static_cast<hipStream_t>(stream));
}

static_assert(sizeof(rm_ball) == 24 && sizeof(RmBall) == sizeof(rm_ball) && offsetof(rm_ball, radius) == 16, "rm_ball layout");
static_assert(sizeof(rm_tiles_update_info) == 32 && sizeof(RmTilesUpdateInfo) == sizeof(rm_tiles_update_info), "rm_tiles_update_info layout");
static_assert(RM_TILES_UPDATE_MAX_BALLS == RM_UPDATE_MAX_BALLS, "the cap on balls");

int rm_scene_tiles_update_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_prev_slot, const void *d_prev_tiles, int64_t n_prev_kept,
                                 const void *d_balls, int32_t n_balls, const void *d_list, int64_t n_kept, void *d_tiles, void *d_reused, void *d_info,
                                 void *stream) {
    if (!ctx) return RM_E_INVALID;
    SparseGrid g;
    if (const char *bad = sparse_error(lattice, &g)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = kept_range_error(g, n_kept)) return fail(ctx, RM_E_INVALID, bad);
    if (n_prev_kept < 0 || n_prev_kept > g.n_blocks) return fail(ctx, RM_E_INVALID, "n_prev_kept must be in [0, n_blocks]");
    if (n_balls < 0 || n_balls > RM_TILES_UPDATE_MAX_BALLS) return fail(ctx, RM_E_INVALID, "n_balls must be in [0, 65536]");
    if (const char *bad = kept_buffers_error(n_kept, d_list, d_tiles)) return fail(ctx, RM_E_INVALID, bad);
    if (n_kept > 0 && !d_prev_slot) return fail(ctx, RM_E_INVALID, "null previous slot map");
    if (n_kept > 0 && n_prev_kept > 0 && !d_prev_tiles) return fail(ctx, RM_E_INVALID, "null previous tiles");
    if (n_balls > 0 && !d_balls) return fail(ctx, RM_E_INVALID, "null balls");
    if (misaligned(d_list, 3) || misaligned(d_prev_slot, 3) || misaligned(d_reused, 3))
        return fail(ctx, RM_E_INVALID, "list, previous slot map and reused must be 4-byte aligned");
    if (misaligned(d_tiles, 7) || misaligned(d_prev_tiles, 7) || misaligned(d_balls, 7) || misaligned(d_info, 7))
        return fail(ctx, RM_E_INVALID, "tiles, previous tiles, balls and info must be 8-byte aligned");
    {  // slots shift when the kept set changes: the update never runs in place
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_tiles), b = reinterpret_cast<uintptr_t>(d_prev_tiles);
        const uintptr_t na = static_cast<uintptr_t>(n_kept) * 8 * RM_SPARSE_TILE, nb = static_cast<uintptr_t>(n_prev_kept) * 8 * RM_SPARSE_TILE;
        if (d_tiles && d_prev_tiles && na && nb && a < b + nb && b < a + na) return fail(ctx, RM_E_INVALID, "tiles and previous tiles overlap");
    }
    if (const int rc = need_device(ctx, "distance path", true)) return rc;
    if (ctx->host.program) return fail(ctx, RM_E_UNSUPPORTED, "expression-program scenes take the full path: rm_scene_tiles_device with option exact");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TilesUpdateCall c{d_prev_slot, d_prev_tiles, d_balls, n_prev_kept, n_balls, d_reused, d_info};
    if (n_kept && (d_reused || !d_info)) {  // nothing of it lives in the scratch
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_tiles_update(ctx, lattice, g, c, d_list, n_kept, d_tiles, s);
    }
    // no kept block, no launch: the totals are zero; else the totals without the caller's flags: the flags live in the scratch
    return scratch_call(ctx, s, n_kept > 0, d_info, sizeof(rm_tiles_update_info), {4 * static_cast<size_t>(n_kept)}, [&](const Staging &st, const size_t *o) {
        c.reused = st.at<void>(o[0]);
        return launch_tiles_update(ctx, lattice, g, c, d_list, n_kept, d_tiles, s);
    });
}

int rm_mesh_tiles_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_slot, const void *d_list, int64_t n_kept, const void *d_tiles, double iso,
                         void *d_vertices, int64_t cap_vertices, void *d_quads, int64_t cap_quads, void *d_cells, void *d_edges, void *d_info,
                         void *stream) {
    if (!ctx) return RM_E_INVALID;
    SparseGrid g;
    if (const char *bad = sparse_error(lattice, &g)) return fail(ctx, RM_E_INVALID, bad);
    const SparseMeshCall m{d_slot, d_list, d_tiles, n_kept, iso, {d_vertices, d_quads, d_cells, d_edges, d_info, cap_vertices, cap_quads}};
    if (const char *bad = kept_range_error(g, n_kept, RM_SPARSE_MAX_KEPT)) return fail(ctx, RM_E_INVALID, bad);
    if (!d_info) return fail(ctx, RM_E_INVALID, "null info");
    if (g.n_blocks > 0 && !d_slot) return fail(ctx, RM_E_INVALID, "null slot");
    if (const char *bad = kept_buffers_error(n_kept, d_list, d_tiles)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = mesh_outputs_error(iso, m.out)) return fail(ctx, RM_E_INVALID, bad);
    if (misaligned(d_slot, 3) || misaligned(d_list, 3)) return fail(ctx, RM_E_INVALID, "slot and list must be 4-byte aligned");
    if (misaligned(d_tiles, 7) || misaligned(d_info, 7)) return fail(ctx, RM_E_INVALID, "tiles and info must be 8-byte aligned");
    if (const int rc = need_device(ctx, "mesher", false)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t k = static_cast<size_t>(n_kept);
    // no kept block, no launch: the totals are zero; else the map and the totals per kept block
    return scratch_call(ctx, s, n_kept > 0, d_info, sizeof(rm_mesh_info), {4 * RM_SPARSE_CELLS * k, 12 * k}, [&](const Staging &st, const size_t *o) {
        return launch_mesh_tiles(ctx, lattice, g, m, st.at<uint32_t>(o[0]), st.at<uint32_t>(o[1]), s);
    });
}

int rm_scene_mesh_sparse(rm_ctx *ctx, const rm_lattice *lattice, double iso, double lipschitz, float *vertices, int64_t cap_vertices, uint32_t *quads,
                         int64_t cap_quads, int64_t *cells, int64_t *edges, rm_mesh_info *info, rm_sparse_info *sparse_info) {
    if (!ctx) return RM_E_INVALID;
    SparseGrid g;
    if (const char *bad = sparse_error(lattice, &g)) return fail(ctx, RM_E_INVALID, bad);
    if (!info) return fail(ctx, RM_E_INVALID, "null info");
    if (!std::isfinite(lipschitz) || !(lipschitz > 0.0)) return fail(ctx, RM_E_INVALID, "lipschitz must be finite and > 0");
    const MeshOutputs host{vertices, quads, cells, edges, info, cap_vertices, cap_quads};
    if (const char *bad = mesh_outputs_error(iso, host)) return fail(ctx, RM_E_INVALID, bad);
    if (const int nrc = need_device(ctx, "mesher", true)) return nrc;
    std::memset(info, 0, sizeof *info);
    rm_sparse_info si;
    std::memset(&si, 0, sizeof si);
    si.n_blocks = g.n_blocks;
    if (sparse_info) *sparse_info = si;
    if (!g.n_blocks) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    // Step 1 in the scratch buffer: the slot map, the list, the info and the scan's totals.
    const size_t nb = static_cast<size_t>(g.n_blocks);
    Staging st{ctx};
    const size_t o_slot = st.region(4 * nb), o_list = st.region(4 * nb), o_sinfo = st.region(sizeof si), o_groups = st.region(4 * sparse_groups(g.n_blocks));
    int rc = st.reserve();
    if (rc) return rc;
    if ((rc = launch_blocks(ctx, lattice, g, iso, lipschitz, st.at<void>(o_slot), st.at<void>(o_list), nullptr, st.at<void>(o_sinfo),
                            st.at<uint32_t>(o_groups), ctx->stream)))
        return rc;
    RM_HIP(ctx, st.out(&si, o_sinfo, sizeof si));
    RM_HIP(ctx, st.sync());
    if (sparse_info) *sparse_info = si;
    const int64_t n_kept = si.n_kept;
    if (n_kept <= 0) return RM_OK;
    if (n_kept > RM_SPARSE_MAX_KEPT) return fail(ctx, RM_E_UNSUPPORTED, "more than 2^21 kept blocks: vertex numbers are 32-bit");
    // Steps 2 and 3 behind the same four regions: the tiles, the mesher's scratch and the outputs; the kept blocks yield a vertex
    // per cell and three quads per cell at most.
    const size_t k = static_cast<size_t>(n_kept);
    const size_t o_tiles = st.region(8 * RM_SPARSE_TILE * k), o_map = st.region(4 * RM_SPARSE_CELLS * k), o_totals = st.region(12 * k);
    const MeshRegions r(st, host, RM_SPARSE_CELLS * n_kept, 3 * RM_SPARSE_CELLS * n_kept);
    if (st.total > ctx->scratch_bytes) {  // the scratch has to grow, which frees it: the map and the list go through the host
        std::vector<int32_t> slot(nb), list(k);
        RM_HIP(ctx, st.out(slot.data(), o_slot, 4 * nb));
        RM_HIP(ctx, st.out(list.data(), o_list, 4 * k));
        RM_HIP(ctx, st.sync());
        if ((rc = st.reserve())) return rc;
        RM_HIP(ctx, st.in(o_slot, slot.data(), 4 * nb));
        RM_HIP(ctx, st.in(o_list, list.data(), 4 * k));
        RM_HIP(ctx, st.sync());  // (the vectors end here)
    }
    if ((rc = launch_tiles(ctx, lattice, g, st.at<void>(o_list), n_kept, st.at<void>(o_tiles), ctx->stream))) return rc;
    const SparseMeshCall m{st.at<void>(o_slot), st.at<void>(o_list), st.at<void>(o_tiles), n_kept, iso, r.on_device(st, host)};
    if ((rc = launch_mesh_tiles(ctx, lattice, g, m, st.at<uint32_t>(o_map), st.at<uint32_t>(o_totals), ctx->stream))) return rc;
    return read_mesh(ctx, st, r, host);
}

int rm_measure_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso, void *d_measure, void *stream) {
    if (!ctx) return RM_E_INVALID;
    int64_t n = 0;
    if (const char *bad = lattice_error(lattice, &n)) return fail(ctx, RM_E_INVALID, bad);
    if (n > (int64_t(1) << 30)) return fail(ctx, RM_E_INVALID, "more than 2^30 lattice points: the measure does not split a volume");
    if (n > 0 && !d_values) return fail(ctx, RM_E_INVALID, "null values");
    if (!d_measure) return fail(ctx, RM_E_INVALID, "null measure");
    if (!std::isfinite(iso)) return fail(ctx, RM_E_INVALID, "non-finite iso");
    if (value_type != RM_MESH_F64 && value_type != RM_MESH_F32) return fail(ctx, RM_E_INVALID, "value_type must be RM_MESH_F64 or RM_MESH_F32");
    if (misaligned(d_values, value_type == RM_MESH_F64 ? 7 : 3)) return fail(ctx, RM_E_INVALID, "values must be aligned to their type");
    if (misaligned(d_measure, 7)) return fail(ctx, RM_E_INVALID, "measure must be 8-byte aligned");
    if (!measure_fits(*lattice, n)) return fail(ctx, RM_E_UNSUPPORTED, kMeasureOverflow);
    if (const int rc = need_device(ctx, "measure", false)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RM_HIP(ctx, hipSetDevice(ctx->device));  // the grid is sized by what this device holds
    const unsigned int groups = rm_measure_field_groups(n, static_cast<unsigned int>(lattice->nv), static_cast<unsigned int>(lattice->nw), ctx->num_cus);
    // one partial per workgroup; without a point the last kernel alone writes the empty record
    return scratch_call(ctx, s, true, d_measure, sizeof(rm_measure), {sizeof(RmMeasurePartial) * groups}, [&](const Staging &st, const size_t *o) {
        return launch_measure_field(ctx, lattice, n, d_values, value_type, iso, st.at<void>(o[0]), groups, d_measure, s);
    });
}

int rm_measure_tiles_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_slot, const void *d_list, int64_t n_kept, const void *d_dist,
                            const void *d_tiles, double iso, void *d_measure, void *stream) {
    if (!ctx) return RM_E_INVALID;
    SparseGrid g;
    if (const char *bad = sparse_error(lattice, &g)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = measure_blocks_error(lattice)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = kept_range_error(g, n_kept)) return fail(ctx, RM_E_INVALID, bad);
    if (!d_measure) return fail(ctx, RM_E_INVALID, "null measure");
    if (!d_slot) return fail(ctx, RM_E_INVALID, "null slot");
    if (!d_dist) return fail(ctx, RM_E_INVALID, "null dist");
    if (const char *bad = kept_buffers_error(n_kept, d_list, d_tiles)) return fail(ctx, RM_E_INVALID, bad);
    if (!std::isfinite(iso)) return fail(ctx, RM_E_INVALID, "non-finite iso");
    if (misaligned(d_slot, 3) || misaligned(d_list, 3)) return fail(ctx, RM_E_INVALID, "slot and list must be 4-byte aligned");
    if (misaligned(d_dist, 7) || misaligned(d_tiles, 7) || misaligned(d_measure, 7)) return fail(ctx, RM_E_INVALID, "dist, tiles and measure must be 8-byte aligned");
    if (!measure_fits(*lattice, g.n)) return fail(ctx, RM_E_UNSUPPORTED, kMeasureOverflow);
    if (const int rc = need_device(ctx, "measure", false)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned int groups = rm_measure_block_groups(static_cast<unsigned int>(g.n_blocks), ctx->num_cus);
    const SparseMeasureCall m{d_slot, d_list, d_dist, d_tiles, n_kept, iso, d_measure};
    // one partial per kept block and per workgroup of the closed forms
    return scratch_call(ctx, s, true, d_measure, sizeof(rm_measure), {sizeof(RmMeasurePartial) * (static_cast<size_t>(n_kept) + groups)},
                        [&](const Staging &st, const size_t *o) { return launch_measure_tiles(ctx, lattice, g, m, st.at<void>(o[0]), groups, s); });
}

int rm_scene_measure(rm_ctx *ctx, const rm_lattice *lattice, double iso, double lipschitz, rm_measure *out, rm_sparse_info *sparse_info) {
    if (!ctx) return RM_E_INVALID;
    SparseGrid g;
    if (const char *bad = sparse_error(lattice, &g)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = measure_blocks_error(lattice)) return fail(ctx, RM_E_INVALID, bad);
    if (!out) return fail(ctx, RM_E_INVALID, "null measure");
    if (!std::isfinite(iso)) return fail(ctx, RM_E_INVALID, "non-finite iso");
    if (!std::isfinite(lipschitz) || !(lipschitz > 0.0)) return fail(ctx, RM_E_INVALID, "lipschitz must be finite and > 0");
    if (!measure_fits(*lattice, g.n)) return fail(ctx, RM_E_UNSUPPORTED, kMeasureOverflow);
    if (const int nrc = need_device(ctx, "measure", true)) return nrc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    // Step 1 in the scratch buffer: the slot map, the list, the distances, the info and the scan's totals.
    const size_t nb = static_cast<size_t>(g.n_blocks);
    Staging st{ctx};
    const size_t o_slot = st.region(4 * nb), o_list = st.region(4 * nb), o_dist = st.region(8 * nb), o_sinfo = st.region(sizeof(rm_sparse_info)),
                 o_groups = st.region(4 * sparse_groups(g.n_blocks));
    int rc = st.reserve();
    if (rc) return rc;
    if ((rc = launch_blocks(ctx, lattice, g, iso, lipschitz, st.at<void>(o_slot), st.at<void>(o_list), st.at<void>(o_dist), st.at<void>(o_sinfo),
                            st.at<uint32_t>(o_groups), ctx->stream)))
        return rc;
    rm_sparse_info si;
    RM_HIP(ctx, st.out(&si, o_sinfo, sizeof si));
    RM_HIP(ctx, st.sync());
    if (sparse_info) *sparse_info = si;
    const int64_t n_kept = si.n_kept;
    if (n_kept < 0 || n_kept > g.n_blocks) return fail(ctx, RM_E_HIP, "the coarse pass reported an impossible n_kept");
    // Steps 2 and 3 behind the same regions: the tiles, the partials and the record.
    const size_t k = static_cast<size_t>(n_kept);
    const unsigned int groups = rm_measure_block_groups(static_cast<unsigned int>(g.n_blocks), ctx->num_cus);
    const size_t o_tiles = st.region(8 * RM_SPARSE_TILE * k), o_partials = st.region(sizeof(RmMeasurePartial) * (k + groups)),
                 o_measure = st.region(sizeof(rm_measure));
    if (st.total > ctx->scratch_bytes) {  // the scratch has to grow, which frees it: step 1's results go through the host
        std::vector<int32_t> slot(nb), list(k);
        std::vector<double> dist(nb);
        RM_HIP(ctx, st.out(slot.data(), o_slot, 4 * nb));
        if (k) RM_HIP(ctx, st.out(list.data(), o_list, 4 * k));
        RM_HIP(ctx, st.out(dist.data(), o_dist, 8 * nb));
        RM_HIP(ctx, st.sync());
        if ((rc = st.reserve())) return rc;
        RM_HIP(ctx, st.in(o_slot, slot.data(), 4 * nb));
        if (k) RM_HIP(ctx, st.in(o_list, list.data(), 4 * k));
        RM_HIP(ctx, st.in(o_dist, dist.data(), 8 * nb));
        RM_HIP(ctx, st.sync());  // (the vectors end here)
    }
    if (k && (rc = launch_tiles(ctx, lattice, g, st.at<void>(o_list), n_kept, st.at<void>(o_tiles), ctx->stream, true))) return rc;
    const SparseMeasureCall m{st.at<void>(o_slot), st.at<void>(o_list), st.at<void>(o_dist), st.at<void>(o_tiles), n_kept, iso, st.at<void>(o_measure)};
    if ((rc = launch_measure_tiles(ctx, lattice, g, m, st.at<void>(o_partials), groups, ctx->stream))) return rc;
    RM_HIP(ctx, st.out(out, o_measure, sizeof *out));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

int rm_measure_world(const rm_lattice *lattice, const rm_measure *measure, struct rm_measure_world *out) {
    int64_t n = 0;
    if (!measure || !out || lattice_error(lattice, &n)) return RM_E_INVALID;
    // binary64, one operation at a time (-ffp-contract=off), in the header's order
    double M[3][3];  // M[p][a]: component p of step a
    for (int p = 0; p < 3; ++p) {
        M[p][0] = static_cast<double>(lattice->du[p]);
        M[p][1] = static_cast<double>(lattice->dv[p]);
        M[p][2] = static_cast<double>(lattice->dw[p]);
    }
    const double u0 = M[0][0], u1 = M[1][0], u2 = M[2][0], v0 = M[0][1], v1 = M[1][1], v2 = M[2][1], w0 = M[0][2], w1 = M[1][2], w2 = M[2][2];
    const double cv = std::fabs((u0 * (v1 * w2 - v2 * w1) - u1 * (v0 * w2 - v2 * w0)) + u2 * (v0 * w1 - v1 * w0));
    const double N = static_cast<double>(measure->n_inside);
    out->cell_volume = cv;
    out->volume = N * cv;
    const double S[3] = {static_cast<double>(measure->sum1[0]), static_cast<double>(measure->sum1[1]), static_cast<double>(measure->sum1[2])};
    const double none = std::numeric_limits<double>::quiet_NaN();  // the mean index of no point
    const bool any = measure->n_inside != 0;
    const double m[3] = {any ? S[0] / N : none, any ? S[1] / N : none, any ? S[2] / N : none};
    for (int c = 0; c < 3; ++c) out->centroid[c] = ((static_cast<double>(lattice->origin[c]) + m[0] * M[c][0]) + m[1] * M[c][1]) + m[2] * M[c][2];
    static const int kPair[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {1, 2}, {2, 0}};  // sum2's order, and second's
    double C[3][3];
    for (int e = 0; e < 6; ++e) {
        const int a = kPair[e][0], b = kPair[e][1];
        C[a][b] = C[b][a] = static_cast<double>(measure->sum2[e]) - (S[a] * S[b]) / N;
    }
    for (int e = 0; e < 6; ++e) {
        const int p = kPair[e][0], q = kPair[e][1];
        if (measure->n_inside == 0) {
            out->second[e] = 0.0;
            continue;
        }
        double t[3];
        for (int a = 0; a < 3; ++a) t[a] = (C[a][0] * M[q][0] + C[a][1] * M[q][1]) + C[a][2] * M[q][2];
        const double pushed = (M[p][0] * t[0] + M[p][1] * t[1]) + M[p][2] * t[2];
        const double own = (M[p][0] * M[q][0] + M[p][1] * M[q][1]) + M[p][2] * M[q][2];
        out->second[e] = pushed * cv + ((N * cv) / 12.0) * own;
    }
    for (int A = 0; A < 3; ++A) {
        const int B = A == 2 ? 0 : A + 1, Cx = A == 0 ? 2 : A - 1;
        const double x = M[1][B] * M[2][Cx] - M[2][B] * M[1][Cx], y = M[2][B] * M[0][Cx] - M[0][B] * M[2][Cx],
                     z = M[0][B] * M[1][Cx] - M[1][B] * M[0][Cx];
        out->projected_area[A] = static_cast<double>(measure->crossings[A]) * std::sqrt((x * x + y * y) + z * z);
    }
    out->area_estimate = (2.0 / 3.0) * ((out->projected_area[0] + out->projected_area[1]) + out->projected_area[2]);
    return RM_OK;
}

// ---- parts: the connected components of one side of iso, and a record each (rm_parts.hip)

static_assert(sizeof(rm_parts_info) == 32 && sizeof(RmPartsInfo) == sizeof(rm_parts_info), "rm_parts_info layout");

namespace {

// what the parts entries check about a lattice of at most 2^30 points, iso and the side; *n receives the point count
const char *parts_error(const rm_lattice *lattice, int64_t *n) {
    if (const char *bad = lattice_error(lattice, n)) return bad;
    return *n > (int64_t(1) << 30) ? "more than 2^30 lattice points: the labelling does not split a volume" : nullptr;
}
const char *parts_side_error(double iso, int32_t side) {
    if (!std::isfinite(iso)) return "non-finite iso";
    return side != RM_PARTS_INSIDE && side != RM_PARTS_OUTSIDE ? "side must be RM_PARTS_INSIDE or RM_PARTS_OUTSIDE" : nullptr;
}
const char *parts_records_error(int64_t n_records, const void *records) {
    if (n_records < 0 || n_records > RM_PARTS_MAX_RECORDS) return "n_records must be in [0, 2^20]";
    return n_records > 0 && !records ? "null records with n_records above 0" : nullptr;
}

// The label launch, n > 0: everything on the device, the info zeroed first -- gave_up is only ever raised.
int launch_label_field(rm_ctx *ctx, const rm_lattice *lat, int64_t n, const void *d_values, int32_t value_type, double iso, int32_t side, void *d_labels,
                       void *d_map, void *d_totals, void *d_info, hipStream_t stream) {
    RmPartsArgs a;
    std::memset(&a, 0, sizeof a);
    a.values = d_values;
    a.iso = iso;
    a.labels = static_cast<int32_t *>(d_labels);
    a.map = static_cast<uint32_t *>(d_map);
    a.totals = static_cast<uint32_t *>(d_totals);
    a.info = static_cast<RmPartsInfo *>(d_info);
    a.n = n;
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
    a.nw = static_cast<unsigned int>(lat->nw);
    a.n_blocks = static_cast<unsigned int>(mesh_blocks(n));
    a.f32 = value_type == RM_MESH_F32;
    a.outside = side == RM_PARTS_OUTSIDE;
    RM_HIP(ctx, hipMemsetAsync(d_info, 0, sizeof(rm_parts_info), stream));
    RM_HIP(ctx, rm_launch_label_field(a, stream, &ctx->last_kernel));
    return RM_OK;
}

int launch_measure_labels(rm_ctx *ctx, const rm_lattice *lat, int64_t n, const void *d_labels, int64_t n_records, void *d_records, hipStream_t stream) {
    RmPartsMeasureArgs a;
    std::memset(&a, 0, sizeof a);
    a.labels = static_cast<const int32_t *>(d_labels);
    a.records = static_cast<RmMeasure *>(d_records);
    a.n = n;
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
    a.nw = static_cast<unsigned int>(lat->nw);
    a.n_records = static_cast<unsigned int>(n_records);
    RM_HIP(ctx, rm_launch_measure_labels(a, ctx->num_cus, stream, &ctx->last_kernel));
    return RM_OK;
}

}  // namespace

int rm_label_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso, int32_t side, void *d_labels,
                          void *d_info, void *stream) {
    if (!ctx) return RM_E_INVALID;
    int64_t n = 0;
    if (const char *bad = parts_error(lattice, &n)) return fail(ctx, RM_E_INVALID, bad);
    if (n > 0 && !d_values) return fail(ctx, RM_E_INVALID, "null values");
    if (const char *bad = parts_side_error(iso, side)) return fail(ctx, RM_E_INVALID, bad);
    if (value_type != RM_MESH_F64 && value_type != RM_MESH_F32) return fail(ctx, RM_E_INVALID, "value_type must be RM_MESH_F64 or RM_MESH_F32");
    if (misaligned(d_values, value_type == RM_MESH_F64 ? 7 : 3)) return fail(ctx, RM_E_INVALID, "values must be aligned to their type");
    if (n > 0 && !d_labels) return fail(ctx, RM_E_INVALID, "null labels");
    if (!d_info) return fail(ctx, RM_E_INVALID, "null info");
    if (misaligned(d_labels, 3)) return fail(ctx, RM_E_INVALID, "labels must be 4-byte aligned");
    if (misaligned(d_info, 7)) return fail(ctx, RM_E_INVALID, "info must be 8-byte aligned");
    if (const int rc = need_device(ctx, "labelling", false)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // no point, no launch: the info is zero; else the map and the block totals, the mesher's layout
    return scratch_call(ctx, s, n > 0, d_info, sizeof(rm_parts_info), {4 * static_cast<size_t>(n), 12 * mesh_blocks(n)},
                        [&](const Staging &st, const size_t *o) {
                            return launch_label_field(ctx, lattice, n, d_values, value_type, iso, side, d_labels, st.at<void>(o[0]), st.at<void>(o[1]), d_info, s);
                        });
}

int rm_measure_labels_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_labels, int64_t n_records, void *d_records, void *stream) {
    if (!ctx) return RM_E_INVALID;
    int64_t n = 0;
    if (const char *bad = parts_error(lattice, &n)) return fail(ctx, RM_E_INVALID, bad);
    if (n > 0 && !d_labels) return fail(ctx, RM_E_INVALID, "null labels");
    if (const char *bad = parts_records_error(n_records, d_records)) return fail(ctx, RM_E_INVALID, bad);
    if (misaligned(d_labels, 3)) return fail(ctx, RM_E_INVALID, "labels must be 4-byte aligned");
    if (misaligned(d_records, 7)) return fail(ctx, RM_E_INVALID, "records must be 8-byte aligned");
    if (!measure_fits(*lattice, n)) return fail(ctx, RM_E_UNSUPPORTED, kMeasureOverflow);
    if (const int rc = need_device(ctx, "measure", false)) return rc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    // the records are the caller's and nothing else is written: no scratch
    return launch_measure_labels(ctx, lattice, n, d_labels, n_records, d_records, static_cast<hipStream_t>(stream));
}

int rm_scene_parts(rm_ctx *ctx, const rm_lattice *lattice, double iso, int32_t side, int32_t *labels_out, int64_t n_records, rm_measure *records_out,
                   rm_parts_info *info_out) {
    if (!ctx) return RM_E_INVALID;
    int64_t n = 0;
    if (const char *bad = parts_error(lattice, &n)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = parts_side_error(iso, side)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = parts_records_error(n_records, records_out)) return fail(ctx, RM_E_INVALID, bad);
    if (!info_out) return fail(ctx, RM_E_INVALID, "null info");
    if (!measure_fits(*lattice, n)) return fail(ctx, RM_E_UNSUPPORTED, kMeasureOverflow);
    int rc = need_device(ctx, "labelling", true);
    if (rc) return rc;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    // The volume, the labels, the labelling's scratch, the info and the records side by side in the scratch buffer.
    const size_t points = static_cast<size_t>(n), records = static_cast<size_t>(n_records);
    Staging st{ctx};
    const size_t o_vol = st.region(8 * points), o_labels = st.region(4 * points), o_map = st.region(4 * points), o_totals = st.region(12 * mesh_blocks(n)),
                 o_info = st.region(sizeof(rm_parts_info)), o_records = st.region(sizeof(rm_measure) * records);
    if ((rc = st.reserve())) return rc;
    if (n > 0) {
        RmRenderParams p;
        RmFieldArgs a;
        fill_field(ctx, lattice, p, a);  // the field entries' own launch, at the lattice's time
        if (const int erc = use_exact(ctx, p)) return erc;
        a.dist = st.at<double>(o_vol);
        a.first = 0;
        a.n = n;
        RM_HIP(ctx, (ctx->opt_length ? rm_launch_field_sqrt : rm_launch_field)(p, a, ctx->stream, &ctx->last_kernel));
        if ((rc = launch_label_field(ctx, lattice, n, st.at<void>(o_vol), RM_MESH_F64, iso, side, st.at<void>(o_labels), st.at<void>(o_map),
                                     st.at<void>(o_totals), st.at<void>(o_info), ctx->stream)))
            return rc;
    } else {
        RM_HIP(ctx, st.zero(o_info, sizeof(rm_parts_info)));
    }
    if ((rc = launch_measure_labels(ctx, lattice, n, st.at<void>(o_labels), n_records, st.at<void>(o_records), ctx->stream))) return rc;
    if (labels_out && n > 0) RM_HIP(ctx, st.out(labels_out, o_labels, 4 * points));
    if (records) RM_HIP(ctx, st.out(records_out, o_records, sizeof(rm_measure) * records));
    RM_HIP(ctx, st.out(info_out, o_info, sizeof *info_out));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

// ---- distances: the exact Euclidean distance transform of one side of iso (rm_edt.hip)

static_assert(sizeof(rm_edt_info) == 32 && sizeof(RmEdtInfo) == sizeof(rm_edt_info), "rm_edt_info layout");
static_assert(RM_EDT_FAR == INT32_MAX, "rm_edt.hip marks an absent parabola with INT_MAX");

namespace {

// every finite squared index distance of the lattice is below RM_EDT_FAR
bool edt_fits(const rm_lattice &l) {
    int64_t sum = 0;
    for (const int64_t count : {int64_t(l.nu), int64_t(l.nv), int64_t(l.nw)}) sum += count > 0 ? (count - 1) * (count - 1) : 0;
    return sum <= int64_t(INT32_MAX) - 1;
}
const char *const kEdtRange = "(nu-1)^2 + (nv-1)^2 + (nw-1)^2 exceeds INT32_MAX - 1: a squared index distance would not fit 32 bits";
const rm_edt_info kEdtEmpty = {0, 0, 0, -1};  // of a lattice without points

// The transform's launch, n > 0: everything on the device; every field of the info is written by the last kernel.
int launch_edt_field(rm_ctx *ctx, const rm_lattice *lat, int64_t n, const void *d_values, int32_t value_type, double iso, int32_t side, void *d_d2,
                     void *d_stack, void *d_partials, void *d_info, hipStream_t stream) {
    RmEdtArgs a;
    std::memset(&a, 0, sizeof a);
    a.values = d_values;
    a.iso = iso;
    a.d2 = static_cast<int32_t *>(d_d2);
    a.stack = static_cast<unsigned long long *>(d_stack);
    a.partials = d_partials;
    a.info = static_cast<RmEdtInfo *>(d_info);
    a.n = n;
    a.nu = static_cast<unsigned int>(lat->nu);
    a.nv = static_cast<unsigned int>(lat->nv);
    a.nw = static_cast<unsigned int>(lat->nw);
    a.f32 = value_type == RM_MESH_F32;
    a.outside = side == RM_PARTS_OUTSIDE;
    RM_HIP(ctx, rm_launch_edt_field(a, stream, &ctx->last_kernel));
    return RM_OK;
}

}  // namespace

int rm_edt_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso, int32_t side, void *d_d2, void *d_info,
                        void *stream) {
    if (!ctx) return RM_E_INVALID;
    int64_t n = 0;
    if (const char *bad = parts_error(lattice, &n)) return fail(ctx, RM_E_INVALID, bad);
    if (n > 0 && !d_values) return fail(ctx, RM_E_INVALID, "null values");
    if (const char *bad = parts_side_error(iso, side)) return fail(ctx, RM_E_INVALID, bad);
    if (value_type != RM_MESH_F64 && value_type != RM_MESH_F32) return fail(ctx, RM_E_INVALID, "value_type must be RM_MESH_F64 or RM_MESH_F32");
    if (misaligned(d_values, value_type == RM_MESH_F64 ? 7 : 3)) return fail(ctx, RM_E_INVALID, "values must be aligned to their type");
    if (n > 0 && !d_d2) return fail(ctx, RM_E_INVALID, "null d2");
    if (!d_info) return fail(ctx, RM_E_INVALID, "null info");
    if (misaligned(d_d2, 3)) return fail(ctx, RM_E_INVALID, "d2 must be 4-byte aligned");
    if (misaligned(d_info, 7)) return fail(ctx, RM_E_INVALID, "info must be 8-byte aligned");
    if (!edt_fits(*lattice)) return fail(ctx, RM_E_UNSUPPORTED, kEdtRange);
    if (const int rc = need_device(ctx, "distance transform", false)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {  // no point, no launch: the info of the empty lattice, which is not all zero
        RM_HIP(ctx, hipSetDevice(ctx->device));
        RM_HIP(ctx, hipMemsetAsync(d_info, 0, offsetof(rm_edt_info, argmax), s));
        RM_HIP(ctx, hipMemsetAsync(static_cast<char *>(d_info) + offsetof(rm_edt_info, argmax), 0xFF, sizeof(int64_t), s));
        return RM_OK;
    }
    // the lines' stacks, laid out as the volume, and the reduction's partials
    return scratch_call(ctx, s, true, d_info, sizeof(rm_edt_info), {8 * static_cast<size_t>(n), RM_EDT_PARTIAL_BYTES}, [&](const Staging &st, const size_t *o) {
        return launch_edt_field(ctx, lattice, n, d_values, value_type, iso, side, d_d2, st.at<void>(o[0]), st.at<void>(o[1]), d_info, s);
    });
}

int rm_scene_edt(rm_ctx *ctx, const rm_lattice *lattice, double iso, int32_t side, int32_t *d2_out, rm_edt_info *info_out) {
    if (!ctx) return RM_E_INVALID;
    int64_t n = 0;
    if (const char *bad = parts_error(lattice, &n)) return fail(ctx, RM_E_INVALID, bad);
    if (const char *bad = parts_side_error(iso, side)) return fail(ctx, RM_E_INVALID, bad);
    if (!info_out) return fail(ctx, RM_E_INVALID, "null info");
    if (!edt_fits(*lattice)) return fail(ctx, RM_E_UNSUPPORTED, kEdtRange);
    int rc = need_device(ctx, "distance transform", true);
    if (rc) return rc;
    if (n == 0) {
        *info_out = kEdtEmpty;
        return RM_OK;
    }
    RM_HIP(ctx, hipSetDevice(ctx->device));
    // The volume, the transform, its stacks and partials and the info side by side in the scratch buffer.
    const size_t points = static_cast<size_t>(n);
    Staging st{ctx};
    const size_t o_vol = st.region(8 * points), o_d2 = st.region(4 * points), o_stack = st.region(8 * points), o_partials = st.region(RM_EDT_PARTIAL_BYTES),
                 o_info = st.region(sizeof(rm_edt_info));
    if ((rc = st.reserve())) return rc;
    RmRenderParams p;
    RmFieldArgs a;
    fill_field(ctx, lattice, p, a);  // the field entries' own launch, at the lattice's time
    if (const int erc = use_exact(ctx, p)) return erc;
    a.dist = st.at<double>(o_vol);
    a.first = 0;
    a.n = n;
    RM_HIP(ctx, (ctx->opt_length ? rm_launch_field_sqrt : rm_launch_field)(p, a, ctx->stream, &ctx->last_kernel));
    if ((rc = launch_edt_field(ctx, lattice, n, st.at<void>(o_vol), RM_MESH_F64, iso, side, st.at<void>(o_d2), st.at<void>(o_stack), st.at<void>(o_partials),
                               st.at<void>(o_info), ctx->stream)))
        return rc;
    if (d2_out) RM_HIP(ctx, st.out(d2_out, o_d2, 4 * points));
    RM_HIP(ctx, st.out(info_out, o_info, sizeof *info_out));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

int rm_lattice_cubic(const rm_lattice *lattice, double *step) {
    int64_t n = 0;
    if (!step || lattice_error(lattice, &n)) return RM_E_INVALID;
    // binary64 of the widened components, one operation at a time (-ffp-contract=off)
    const float *const steps[3] = {lattice->du, lattice->dv, lattice->dw};
    const int32_t counts[3] = {lattice->nu, lattice->nv, lattice->nw};
    double v[3][3], first = 1.0;
    int m = 0;  // the axes that take part: those with more than one point
    for (int A = 0; A < 3; ++A) {
        if (counts[A] <= 1) continue;
        for (int c = 0; c < 3; ++c) v[m][c] = static_cast<double>(steps[A][c]);
        ++m;
    }
    const auto dot = [&](int p, int q) { return (v[p][0] * v[q][0] + v[p][1] * v[q][1]) + v[p][2] * v[q][2]; };
    if (m > 0) first = std::sqrt(dot(0, 0));
    for (int p = 1; p < m; ++p)
        if (!(std::fabs(std::sqrt(dot(p, p)) - first) <= 1e-5 * first)) return RM_E_UNSUPPORTED;
    for (int p = 0; p < m; ++p)
        for (int q = p + 1; q < m; ++q)
            if (!(std::fabs(dot(p, q)) <= 1e-5 * (first * first))) return RM_E_UNSUPPORTED;
    *step = first;
    return RM_OK;
}

int rm_debug_wave_distance(rm_ctx *ctx, const float *points_xyz, int64_t n, double *dist, uint32_t *count) {
    RmRenderParams p;
    const auto supported = [&] {
        rm_ray_query q;
        std::memset(&q, 0, sizeof q);
        q.algorithm = RM_ALG_SPHERE_TRACER;
        q.time = ctx->time;
        q.overshoot_factor = q.step_size = std::numeric_limits<double>::quiet_NaN();
        const int rc = fill_query_params(ctx, &q, p);  // every option applies as it does to a render of the active scene
        if (rc) return rc;
        if (p.accel != RM_ACCEL_BVH || p.general || p.bvh_nodes <= 0) return fail(ctx, RM_E_UNSUPPORTED, "the wave loop's distance query serves BVH sphere scenes");
        return static_cast<int>(RM_OK);
    };
    return points_call(ctx, points_xyz, n, dist, count, supported, [&](const float *d_points, double *d_dist, uint32_t *d_count) {
        return (ctx->opt_length ? rm_launch_wave_distance_sqrt : rm_launch_wave_distance)(p, d_points, n, d_dist, d_count, ctx->stream);
    });
}

int rm_ray_march_device(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *d_origins, const void *d_dirs, void *d_t, void *d_iters,
                        void *d_sdf_calls, void *d_normal, void *stream) {
    return ray_call<RmQueryArgs>(ctx, q, n, d_origins, d_dirs, false, stream, no_check,
                                 [&](RayCall<RmQueryArgs> &c) { query_call(c, ctx, q, false, d_t, d_iters, d_sdf_calls, d_normal, nullptr); });
}

int rm_ray_march(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const float *origins_xyz, const float *dirs_xyz, double *t, uint32_t *iters,
                 uint32_t *sdf_calls, float *normal_xyz) {
    return ray_call<RmQueryArgs>(ctx, q, n, origins_xyz, dirs_xyz, true, nullptr, no_check,
                                 [&](RayCall<RmQueryArgs> &c) { query_call(c, ctx, q, false, t, iters, sdf_calls, normal_xyz, nullptr); });
}

int rm_camera_rays(int32_t width, int32_t height, double pitch, double yaw, int32_t y_start, int32_t y_end, float *origin3, float *dirs_xyz) {
    if (width < 0 || height <= 0 || y_start < 0 || y_end < y_start || y_end > height) return RM_E_INVALID;
    if (!std::isfinite(pitch) || !std::isfinite(yaw) || !origin3) return RM_E_INVALID;
    const int64_t npx = static_cast<int64_t>(y_end - y_start) * width;
    if (npx > 0 && !dirs_xyz) return RM_E_INVALID;
    float rot[9];
    rmh::camera_from_angles(pitch, yaw, rot, origin3);
    for (int32_t y = y_start; y < y_end; ++y) {
        const double v = (static_cast<double>(y) / height - 0.5) * 2.0;  // raymarcher.ts:73
        for (int32_t x = 0; x < width; ++x) {
            const double u = (static_cast<double>(x) / width - 0.5) * 2.0;                        // :83
            const double ax = static_cast<float>(u), ay = static_cast<float>(v), az = -1.0;       // :84 vec3.fromValues
            const float dx = static_cast<float>(ax * rot[0] + ay * rot[3] + az * rot[6]);         // :87 vec3.transformMat3
            const float dy = static_cast<float>(ax * rot[1] + ay * rot[4] + az * rot[7]);
            const float dz = static_cast<float>(ax * rot[2] + ay * rot[5] + az * rot[8]);
            double len = static_cast<double>(dx) * dx + static_cast<double>(dy) * dy + static_cast<double>(dz) * dz;  // :88 vec3.normalize
            if (len > 0) len = 1 / std::sqrt(len);
            float *o = dirs_xyz + 3 * (static_cast<int64_t>(y - y_start) * width + x);
            o[0] = static_cast<float>(dx * len);
            o[1] = static_cast<float>(dy * len);
            o[2] = static_cast<float>(dz * len);
        }
    }
    return RM_OK;
}

int rm_ray_pick_device(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *d_origins, const void *d_dirs, void *d_t, void *d_iters,
                       void *d_sdf_calls, void *d_normal, void *d_object, void *stream) {
    return ray_call<RmQueryArgs>(ctx, q, n, d_origins, d_dirs, false, stream, no_check,
                                 [&](RayCall<RmQueryArgs> &c) { query_call(c, ctx, q, true, d_t, d_iters, d_sdf_calls, d_normal, d_object); });
}

int rm_ray_pick(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const float *origins_xyz, const float *dirs_xyz, double *t, uint32_t *iters,
                uint32_t *sdf_calls, float *normal_xyz, int32_t *object) {
    return ray_call<RmQueryArgs>(ctx, q, n, origins_xyz, dirs_xyz, true, nullptr, no_check,
                                 [&](RayCall<RmQueryArgs> &c) { query_call(c, ctx, q, true, t, iters, sdf_calls, normal_xyz, object); });
}

int rm_ray_light_device(rm_ctx *ctx, const rm_ray_query *q, const rm_light *light, int64_t n, const void *d_origins, const void *d_dirs, void *d_t,
                        void *d_iters, void *d_sdf_calls, void *d_normal, void *d_lit, void *d_ao, void *d_iters2, void *d_sdf_calls2,
                        void *stream) {
    return ray_call<RmLightArgs>(ctx, q, n, d_origins, d_dirs, false, stream, [&] { return check_light(ctx, light); },
                                 [&](RayCall<RmLightArgs> &c) { light_call(c, light, d_t, d_iters, d_sdf_calls, d_normal, d_lit, d_ao, d_iters2, d_sdf_calls2); });
}

int rm_ray_light(rm_ctx *ctx, const rm_ray_query *q, const rm_light *light, int64_t n, const float *origins_xyz, const float *dirs_xyz, double *t,
                 uint32_t *iters, uint32_t *sdf_calls, float *normal_xyz, float *lit, float *ao, uint32_t *iters2, uint32_t *sdf_calls2) {
    return ray_call<RmLightArgs>(ctx, q, n, origins_xyz, dirs_xyz, true, nullptr, [&] { return check_light(ctx, light); },
                                 [&](RayCall<RmLightArgs> &c) { light_call(c, light, t, iters, sdf_calls, normal_xyz, lit, ao, iters2, sdf_calls2); });
}

int rm_ray_walk_device(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *d_origins, const void *d_dirs, int32_t cap, void *d_walks,
                       void *d_steps, void *stream) {
    return ray_call<RmWalkArgs>(ctx, q, n, d_origins, d_dirs, false, stream, [&] { return check_walk(ctx, true, n, cap, d_walks, d_steps); },
                                [&](RayCall<RmWalkArgs> &c) { walk_call(c, cap, d_walks, d_steps); });
}

int rm_ray_walk(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const float *origins_xyz, const float *dirs_xyz, int32_t cap, rm_walk *walks,
                rm_step *steps) {
    return ray_call<RmWalkArgs>(ctx, q, n, origins_xyz, dirs_xyz, true, nullptr, [&] { return check_walk(ctx, false, n, cap, walks, steps); },
                                [&](RayCall<RmWalkArgs> &c) { walk_call(c, cap, walks, steps); });
}

int rm_phong_light(float dir3[3]) {
    if (!dir3) return RM_E_INVALID;
    rmh::phong_light_dir(dir3);
    return RM_OK;
}

int rm_scene_object(rm_ctx *ctx, int32_t index, rm_node *nodes, int32_t cap, int32_t *n_nodes) {
    if (!ctx) return RM_E_INVALID;
    if (n_nodes) *n_nodes = 0;
    if (cap < 0 || (cap > 0 && !nodes)) return fail(ctx, RM_E_INVALID, "bad node buffer");
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    if (index < 0 || index >= scene_n_prims(ctx)) return fail(ctx, RM_E_INVALID, "object index out of range");
    std::vector<rm_node> tree;
    object_forest(ctx, index, tree);
    if (tree.empty()) return fail(ctx, RM_E_UNSUPPORTED, "the active scene keeps no description of its objects");
    const int32_t need = static_cast<int32_t>(tree.size());
    if (n_nodes) *n_nodes = need;
    if (need <= cap) std::memcpy(nodes, tree.data(), tree.size() * sizeof(rm_node));
    return RM_OK;
}

int rm_selftest_hypot(rm_ctx *ctx, const float *xyz, int64_t n, double *out) {
    RM_NEED_DEVICE(ctx, "host-only context");
    if (n < 0 || (n > 0 && (!xyz || !out))) return fail(ctx, RM_E_INVALID, "bad buffers");
    if (!n) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t k = static_cast<size_t>(n);
    Staging st{ctx};
    const size_t o_xyz = st.region(12 * k), o_out = st.region(8 * k);
    int rc = st.reserve();
    if (rc) return rc;
    RM_HIP(ctx, st.in(o_xyz, xyz, 12 * k));
    RM_HIP(ctx, rm_launch_hypot(st.at<const float>(o_xyz), n, st.at<double>(o_out), ctx->stream));
    RM_HIP(ctx, st.out(out, o_out, 8 * k));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

int rm_selftest_jsmath(rm_ctx *ctx, int32_t fn, const double *a, const double *b, int64_t n, double *out) {
    RM_NEED_DEVICE(ctx, "host-only context");
    if (n < 0 || fn < 0 || fn > 7 || (n > 0 && (!a || !out))) return fail(ctx, RM_E_INVALID, "bad buffers");
    if (!n) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t k = static_cast<size_t>(n);
    Staging st{ctx};
    const size_t o_a = st.region(8 * k), o_b = st.region(8 * k), o_out = st.region(8 * k);
    int rc = st.reserve();
    if (rc) return rc;
    RM_HIP(ctx, st.in(o_a, a, 8 * k));
    if (b) RM_HIP(ctx, st.in(o_b, b, 8 * k));
    else RM_HIP(ctx, st.zero(o_b, 8 * k));  // no second operand: zeros
    RM_HIP(ctx, rm_launch_jsmath(fn, st.at<const double>(o_a), st.at<const double>(o_b), n, st.at<double>(o_out), ctx->stream));
    RM_HIP(ctx, st.out(out, o_out, 8 * k));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

int rm_selftest_hypot64(rm_ctx *ctx, const double *xyz, int64_t n, int32_t on_device, double *out) {
    if (!ctx) return RM_E_INVALID;
    if (n < 0 || (n > 0 && (!xyz || !out))) return fail(ctx, RM_E_INVALID, "bad buffers");
    if (!on_device) {  // the host builder's own Math.hypot
        for (int64_t i = 0; i < n; ++i) out[i] = rmh::js_hypot3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        return RM_OK;
    }
    if (!ctx->has_device) return fail(ctx, RM_E_NO_DEVICE, "host-only context");
    if (!n) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t k = static_cast<size_t>(n);
    Staging st{ctx};
    const size_t o_xyz = st.region(24 * k), o_out = st.region(8 * k);
    int rc = st.reserve();
    if (rc) return rc;
    RM_HIP(ctx, st.in(o_xyz, xyz, 24 * k));
    RM_HIP(ctx, rm_launch_hypot64(st.at<const double>(o_xyz), n, st.at<double>(o_out), ctx->stream));
    RM_HIP(ctx, st.out(out, o_out, 8 * k));
    RM_HIP(ctx, st.sync());
    return RM_OK;
}

int rm_selftest_fastdiv(rm_ctx *ctx, uint64_t seed, int64_t n, uint64_t *mismatches) {
    if (!mismatches) return RM_E_INVALID;
    RM_NEED_DEVICE(ctx, "host-only context");
    if (n < 0) return fail(ctx, RM_E_INVALID, "negative count");
    return read_mismatches(ctx, [&](unsigned long long *d) { return rm_launch_fastdiv_selftest(seed, n, d, ctx->stream); }, mismatches);
}

int rm_selftest_recip(rm_ctx *ctx, int mode, uint64_t *mismatches) {
    if (!mismatches) return RM_E_INVALID;
    RM_NEED_DEVICE(ctx, "host-only context");
    if (mode != 0 && mode != 1) return fail(ctx, RM_E_INVALID, "mode must be 0 or 1");
    return read_mismatches(ctx, [&](unsigned long long *d) { return rm_launch_recip_selftest(mode, d, ctx->stream); }, mismatches);
}

// The rm_debug_read_* entries of the diagnostic builds (-DRM_STAMPS, -DRM_COUNTS, ...): `bytes` of ctx->d_stamps from word
// `first` on, read behind everything enqueued and zeroed for the next launch.
static int read_stamps(rm_ctx *ctx, void *out, size_t first, size_t bytes) {
    if (!out) return RM_E_INVALID;
    RM_NEED_DEVICE(ctx, "host-only context");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RM_HIP(ctx, hipDeviceSynchronize());
    RM_HIP(ctx, hipMemcpy(out, ctx->d_stamps + first, bytes, hipMemcpyDeviceToHost));
    RM_HIP(ctx, hipMemset(ctx->d_stamps + first, 0, bytes));
    return RM_OK;
}

int rm_debug_read_stamps(rm_ctx *ctx, uint64_t *out8) {
    const int rc = read_stamps(ctx, out8, 0, 8 * sizeof(uint64_t));
    if (rc) return rc;
    RM_HIP(ctx, hipMemset(ctx->d_stamps + 6, 0xFF, sizeof(uint64_t)));  // slot 6: minimum start time of the next launch's waves
    return RM_OK;
}

// -DRM_STAMPS builds: start / end time (s_memrealtime, 100 MHz) of the first 8192 waves of the last v2 launch
int rm_debug_read_wave_times(rm_ctx *ctx, uint64_t *out16384) { return read_stamps(ctx, out16384, 40, 3 * 8192 * sizeof(uint64_t)); }

// -DRM_STAMPS -DRM_STAMPS_LOG builds: the low 32 bits of s_memrealtime at the start of the first 96 batches of the first 2048 waves
int rm_debug_read_batch_log(rm_ctx *ctx, uint32_t *out196608) { return read_stamps(ctx, out196608, 40 + 3 * 8192, 2048 * 96 * sizeof(uint32_t)); }

int rm_debug_read_counts(rm_ctx *ctx, uint64_t *out32) { return read_stamps(ctx, out32, 8, 32 * sizeof(uint64_t)); }

// ---- run-time specialisation of expression forests (rm_rtc.h) -------------------------------------------------------------
static int copy_text(const std::string &t, char *out, int64_t cap, int64_t *needed) {
    if (needed) *needed = static_cast<int64_t>(t.size()) + 1;
    if (out && cap > 0) {
        const size_t n = std::min(static_cast<size_t>(cap - 1), t.size());
        std::memcpy(out, t.data(), n);
        out[n] = '\0';
    }
    return RM_OK;
}

int rm_rtc_source(rm_ctx *ctx, char *out, int64_t cap, int64_t *needed) {
    if (!ctx) return RM_E_INVALID;
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene");
    return copy_text(ctx->rtc_src, out, cap, needed);
}

int rm_rtc_compile_check(rm_ctx *ctx, int32_t accel, int32_t other, char *log, int64_t cap, double *seconds) {
    if (!ctx) return RM_E_INVALID;
    if (!ctx->have_scene || ctx->rtc_src.empty()) return fail(ctx, RM_E_NO_SCENE, "the active scene has no specialised source");
    rmrtc::Kernel k;
    std::string text;
    const bool ok = rmrtc::compile(ctx->rtc_src, norm_accel(accel), other != 0, ctx->opt_length != 0, false, k, text);
    if (seconds) *seconds = k.compile_seconds;
    copy_text(text, log, cap, nullptr);
    if (ok) return RM_OK;
    if (text.compare(0, 8, "refused:") == 0) return fail(ctx, RM_E_UNSUPPORTED, "hiprtc: the specialised kernel spills and would not be loaded (see the log)");
    return fail(ctx, RM_E_INVALID, "hiprtc: the specialised kernel did not compile (see the log)");
}

int rm_rtc_status(rm_ctx *ctx, int32_t *compiled, int32_t *failed, char *log, int64_t cap) {
    if (!ctx) return RM_E_INVALID;
    int v2_ready = 0, v2_failed = 0;
    for (const auto &kv : ctx->v2_special) {
        v2_ready += kv.second.state == 1;
        v2_failed += kv.second.state < 0;
    }
    if (compiled) *compiled = static_cast<int32_t>(ctx->rtc_kernels.size()) + v2_ready;
    if (failed) *failed = static_cast<int32_t>(ctx->rtc_failed.size()) + v2_failed;
    std::string why;
    if (!rmrtc::available(&why)) return copy_text(why, log, cap, nullptr);
    return copy_text(ctx->rtc_log, log, cap, nullptr);
}

// the item costs (durations in units of 2.56 us, one byte per item, 64 queues x LptRing::kStride slots) the LAST v2 launch recorded
int rm_debug_read_lpt_costs(rm_ctx *ctx, uint8_t *out, int64_t n) {
    if (!out) return RM_E_INVALID;
    RM_NEED_DEVICE(ctx, "host-only context");
    const uint8_t *costs = ctx->lpt.last_costs();
    if (!costs || n < 0 || static_cast<size_t>(n) > LptRing::kPerSlot) return fail(ctx, RM_E_INVALID, "no costs recorded");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RM_HIP(ctx, hipDeviceSynchronize());
    RM_HIP(ctx, hipMemcpy(out, costs, static_cast<size_t>(n), hipMemcpyDeviceToHost));
    return RM_OK;
}

// what a v2 launch that asks for `asked` workgroups per CU would bring (launch_fill: option `min_fill`, the queue count rm_create read)
int rm_debug_launch_fill(rm_ctx *ctx, int32_t asked, int32_t *effective) {
    if (!ctx || !effective) return RM_E_INVALID;
    if (asked < 1 || asked > 8) return fail(ctx, RM_E_INVALID, "blocks_per_cu must be in [1, 8]");
    *effective = launch_fill(asked, ctx->hw_queues, ctx->opt_min_fill != 0);
    return RM_OK;
}

// ... and what it brings for a frame of `items` work items (overlap_fill above, rm_v2_overlap_per_cu): options `min_fill` and
// `overlap_fill`, the queue count rm_create read, the context's CU count (256 without a device)
int rm_debug_overlap_fill(rm_ctx *ctx, int32_t asked, int64_t items, int32_t *effective) {
    if (!ctx || !effective) return RM_E_INVALID;
    if (asked < 1 || asked > 8) return fail(ctx, RM_E_INVALID, "blocks_per_cu must be in [1, 8]");
    if (items < 0) return fail(ctx, RM_E_INVALID, "items must not be negative");
    const bool min_fill = ctx->opt_min_fill != 0;
    *effective = rm_v2_overlap_per_cu(launch_fill(asked, ctx->hw_queues, min_fill),
                                      overlap_fill(asked, ctx->hw_queues, min_fill, ctx->opt_overlap_fill != 0), items, ctx->num_cus);
    return RM_OK;
}

// the last launch of the v2 wave loop: workgroups, threads per workgroup, dynamic LDS bytes (zeros before the first); the context's CU count
int rm_debug_last_launch(rm_ctx *ctx, uint32_t out[4]) {
    if (!ctx || !out) return RM_E_INVALID;
    for (int k = 0; k < 3; ++k) out[k] = ctx->last_v2_shape[k];
    out[3] = static_cast<uint32_t>(ctx->num_cus);
    return RM_OK;
}

// Section M of the v2 wave loop and the step-box table (option `step_box`), without a device: out[0] whether the last v2 launch
// tested its in-round steps against the table (0 before the first), out[1] whether a launch of the active scene under the
// options as they stand would (the launcher's own decision, rm_v2_plan), out[2] why not -- 0 it would, 1 the options (`step_box`,
// `multi_step`, `kernel`) or the scene's kind rule it out, 2 the scene has no table, 3 the table would cost LDS the launch
// keeps for something else -- out[3] the hit-list capacity that launch gets and out[4] the one it would get with `step_box` 0,
// out[5] the table's size in bytes.
int rm_debug_step_box(rm_ctx *ctx, int32_t out[6]) {
    if (!ctx || !out) return RM_E_INVALID;
    for (int k = 0; k < 6; ++k) out[k] = 0;
    out[0] = static_cast<int32_t>(ctx->last_v2_shape[3]);
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    rm_job job;
    std::memset(&job, 0, sizeof job);
    job.width = job.height = job.y_end = 64;
    job.algorithm = RM_ALG_SPHERE_TRACER;
    job.scene_preset_index = ctx->scene_is_uploaded ? RM_SCENE_UPLOADED : ctx->scene_preset;
    job.acceleration_structure = ctx->host.accel;
    job.overshoot_factor = job.step_size = std::nan("");
    const double scene_time = ctx->time;
    RmRenderParams p;
    const int rc = fill_params(ctx, &job, p);
    ctx->time = scene_time;  // (a debug read leaves the scene's time alone)
    if (rc) return rc;
    out[5] = static_cast<int32_t>(ctx->host.step_tab.size() * sizeof(uint32_t));
    RmRenderParams plain = p;
    plain.step_box = 0;
    out[4] = rm_v2_plan(plain).list_cap;
    const RmV2Plan plan = rm_v2_plan(p);
    out[3] = plan.list_cap;
    const bool v2 = p.variant == 2 && p.algorithm == 0 && p.accel == 2;
    out[1] = v2 && plan.step_box ? 1 : 0;
    out[2] = out[1] ? 0 : (ctx->host.step_tab.empty() && v2 && ctx->opt_step_box && ctx->opt_multi_step ? 2 : (v2 && plan.refused ? 3 : 1));
    return RM_OK;
}

// Sections B and M of the v2 wave loop and the scene's cell table (option `cell_tab`), without a device: out[0] whether the last
// v2 launch read its candidates from the table (0 before the first), out[1] whether a launch of the active scene under the
// options as they stand would (rm_v2_plan), out[2] why not -- 0 it would, 1 the options (`cell_tab`, `step_box`, `multi_step`,
// `kernel`), the kind of scene or a launch without the step-box table rule it out, 2 the scene has no table, 3 the table would
// cost the launch a workgroup per CU, hit-list entries or its staging -- out[3] the hit-list capacity that launch gets and
// out[4] the one it would get with `cell_tab` 0, out[5] the table's size in bytes, out[6] the workgroups of that launch a CU
// holds by its LDS, out[7] / out[8] the bytes of scene tables it stages and would stage with `cell_tab` 0, out[9] the table's
// cells, out[10] its records, out[11] its distinct leaf sets.
int rm_debug_cell_tab(rm_ctx *ctx, int32_t out[12]) {
    if (!ctx || !out) return RM_E_INVALID;
    for (int k = 0; k < 12; ++k) out[k] = 0;
    out[0] = static_cast<int32_t>(ctx->last_v2_shape[5]);
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    rm_job job;
    std::memset(&job, 0, sizeof job);
    job.width = job.height = job.y_end = 64;
    job.algorithm = RM_ALG_SPHERE_TRACER;
    job.scene_preset_index = ctx->scene_is_uploaded ? RM_SCENE_UPLOADED : ctx->scene_preset;
    job.acceleration_structure = ctx->host.accel;
    job.overshoot_factor = job.step_size = std::nan("");
    const double scene_time = ctx->time;
    RmRenderParams p;
    const int rc = fill_params(ctx, &job, p);
    ctx->time = scene_time;  // (a debug read leaves the scene's time alone)
    if (rc) return rc;
    const auto &tab = ctx->host.cell_tab;
    out[5] = static_cast<int32_t>(tab.size() * sizeof(uint32_t));
    if (!tab.empty()) {
        out[9] = static_cast<int32_t>(tab[0] * tab[1] * tab[2]);
        out[10] = static_cast<int32_t>(tab[3]);
        out[11] = static_cast<int32_t>(tab[7]);
    }
    RmRenderParams plain = p;
    plain.cell_on = 0;
    const RmV2Plan without = rm_v2_plan(plain);
    out[4] = without.list_cap;
    out[8] = static_cast<int32_t>(without.lds ? without.scene_bytes : 0);
    const RmV2Plan plan = rm_v2_plan(p);
    out[3] = plan.list_cap;
    out[6] = plan.per_cu;
    out[7] = static_cast<int32_t>(plan.lds ? plan.scene_bytes : 0);
    const bool v2 = p.variant == 2 && p.algorithm == 0 && p.accel == 2;
    out[1] = v2 && plan.cell_on ? 1 : 0;
    out[2] = out[1] ? 0 : (tab.empty() && v2 && ctx->opt_cell_tab && ctx->opt_step_box && ctx->opt_multi_step ? 2 : (v2 && plan.cell_refused ? 3 : 1));
    return RM_OK;
}

// Section M's runner-up test (option `runner_up`), without a device: out[0] whether the last v2 launch bounded the runner-up by
// its own distance (0 before the first), out[1] whether a launch of the active scene under the options as they stand would
// (rm_v2_plan), out[2] why not -- 0 it would, 1 option `runner_up` is 0, 2 the launch does not take the cell table
// (rm_debug_cell_tab says why), 3 the scene's spheres do not share one radius (or option `uniform` is 0).
int rm_debug_runner_up(rm_ctx *ctx, int32_t out[4]) {
    if (!ctx || !out) return RM_E_INVALID;
    for (int k = 0; k < 4; ++k) out[k] = 0;
    out[0] = static_cast<int32_t>(ctx->last_v2_shape[6]);
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    rm_job job;
    std::memset(&job, 0, sizeof job);
    job.width = job.height = job.y_end = 64;
    job.algorithm = RM_ALG_SPHERE_TRACER;
    job.scene_preset_index = ctx->scene_is_uploaded ? RM_SCENE_UPLOADED : ctx->scene_preset;
    job.acceleration_structure = ctx->host.accel;
    job.overshoot_factor = job.step_size = std::nan("");
    const double scene_time = ctx->time;
    RmRenderParams p;
    const int rc = fill_params(ctx, &job, p);
    ctx->time = scene_time;  // (a debug read leaves the scene's time alone)
    if (rc) return rc;
    const RmV2Plan plan = rm_v2_plan(p);
    const bool v2 = p.variant == 2 && p.algorithm == 0 && p.accel == 2;
    out[1] = v2 && plan.runner_up ? 1 : 0;
    out[2] = out[1] ? 0 : (!ctx->opt_runner_up ? 1 : (!(v2 && plan.cell_on) ? 2 : 3));
    return RM_OK;
}

// The three-key update of the one-radius scan (rm_kernels.h rm_scan_keys_update, the text the wave loop runs) over a caller's
// list of n keys, without a device: out3[0 .. 2] the three smallest in order (all ones where there are fewer), *lb3 the third
// key's bound for radius rf (rm_scan_key_bound: +inf exactly when fewer than three keys came), *lb3_carried that bound as section
// M reads it after its trip through the upper half of a word (rm_runner_up_pack_bound / _unpack_bound).  `keys` may be null when n is 0.
int rm_debug_scan_keys(const uint32_t *keys, int64_t n, float rf, uint32_t out3[3], float *lb3, float *lb3_carried) {
    if (n < 0 || (n > 0 && !keys) || !out3 || !lb3 || !lb3_carried) return RM_E_INVALID;
    RmScanKeys k = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (int64_t i = 0; i < n; ++i) rm_scan_keys_update(k, keys[i]);
    out3[0] = k.best;
    out3[1] = k.second;
    out3[2] = k.third;
    *lb3 = rm_scan_key_bound(k.third, rf);
    *lb3_carried = rm_runner_up_unpack_bound(rm_runner_up_pack_bound(*lb3));
    return RM_OK;
}

// What the next exact query (option `exact`) of the active scene walks, without a device: out[0] the mode (0 every object, 1 the
// scene's BVH, 2 an own tree), out[1 .. 3] the nodes, leaves and depth of that tree (zeros in mode 0).  Builds the own tree if
// it is due, whatever the option says.
int rm_debug_exact_tree(rm_ctx *ctx, int32_t out[4]) {
    if (!ctx || !out) return RM_E_INVALID;
    for (int k = 0; k < 4; ++k) out[k] = 0;
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    const int rc = ensure_exact_tree(ctx);
    if (rc) return rc;
    out[0] = ctx->exact_mode;
    if (ctx->exact_mode == 1) {
        out[1] = static_cast<int32_t>(ctx->host.bvh.size());
        out[2] = ctx->host.bvh_leaves;
        out[3] = ctx->host.bvh_depth;
    } else if (ctx->exact_mode == 2) {
        out[1] = static_cast<int32_t>(ctx->exact_tree.nodes.size());
        out[2] = ctx->exact_tree.leaves;
        out[3] = ctx->exact_tree.depth;
    }
    return RM_OK;
}

// The leaf rectangles of the bundle cull (option `rect_cull`), without a device.  `rot9` / `origin3`: the camera
// (rm_camera_from_angles gives a job's), width x height the full frame.  out[0] whether the last v2 launch culled by
// rectangles (0 before the first), out[1] whether a launch of the active scene with this camera and frame would, out[2] why
// not (rect_cull_refusal above; 1 also when the options or the scene keep the launch out of the wave loop), out[3] the
// scene's leaves in the cull's table, out[4] the most a launch keeps rectangles for.
int rm_debug_rect_cull(rm_ctx *ctx, const float *rot9, const float *origin3, int32_t width, int32_t height, int32_t out[5]) {
    if (!ctx || !out || !rot9 || !origin3) return RM_E_INVALID;
    for (int k = 0; k < 5; ++k) out[k] = 0;
    out[0] = static_cast<int32_t>(ctx->last_v2_shape[4]);
    out[4] = RM_RECT_CULL_MAX_LEAVES;
    if (!ctx->have_scene) return fail(ctx, RM_E_NO_SCENE, "no scene set");
    rm_job job;
    std::memset(&job, 0, sizeof job);
    job.width = job.height = job.y_end = 64;
    job.algorithm = RM_ALG_SPHERE_TRACER;
    job.scene_preset_index = ctx->scene_is_uploaded ? RM_SCENE_UPLOADED : ctx->scene_preset;
    job.acceleration_structure = ctx->host.accel;
    job.overshoot_factor = job.step_size = std::nan("");
    const double scene_time = ctx->time;
    RmRenderParams p;
    const int rc = fill_params(ctx, &job, p);
    ctx->time = scene_time;  // (a debug read leaves the scene's time alone)
    if (rc) return rc;
    out[3] = static_cast<int32_t>(ctx->cull_leaves.size());
    const bool v2 = p.variant == 2 && p.algorithm == 0 && p.accel == 2;
    out[2] = v2 ? rect_cull_refusal(ctx, rot9, origin3, width, height) : 1;
    out[1] = out[2] == 0 ? 1 : 0;
    return RM_OK;
}

// The table such a launch's workgroups fill (rm_kernels.h rm_leaf_rect, the text the kernel runs), on the host: entry j, four
// uint16 x_lo, x_hi, y_lo, y_hi, for node nodes[j] of the scene's BVH.  *n: the entries there are -- 0 when the launch would
// take the plane cull (rm_debug_rect_cull says why) -- of which the first `cap` are written.  `rects` and `nodes` may be null.
int rm_debug_leaf_rects(rm_ctx *ctx, const float *rot9, const float *origin3, int32_t width, int32_t height, uint16_t *rects,
                        int32_t *nodes, int64_t cap, int64_t *n) {
    if (!ctx || !n || !rot9 || !origin3 || cap < 0) return RM_E_INVALID;
    *n = 0;
    int32_t why[5];
    const int rc = rm_debug_rect_cull(ctx, rot9, origin3, width, height, why);
    if (rc) return rc;
    if (!why[1]) return RM_OK;
    *n = static_cast<int64_t>(ctx->cull_leaves.size());
    for (int64_t j = 0; j < *n && j < cap; ++j) {
        const RmBvhNode &nd = ctx->host.bvh[ctx->cull_leaves[static_cast<size_t>(j)]];
        const RmLeafRect r = rm_leaf_rect(nd.lo, nd.hi, origin3, rot9, width, height);
        if (rects) {
            rects[4 * j] = r.x_lo;
            rects[4 * j + 1] = r.x_hi;
            rects[4 * j + 2] = r.y_lo;
            rects[4 * j + 3] = r.y_hi;
        }
        if (nodes) nodes[j] = ctx->cull_leaves[static_cast<size_t>(j)];
    }
    return RM_OK;
}

// Every option once: its key, its member of rm_ctx (the defaults and what they were measured against are there; fill_params
// reads the members), the values it takes and what rm_last_error says of any other.
enum OptionKind {
    kSwitch,       // 0 | 1: any non-zero value is 1
    kRange,        // v[0] .. v[1], inclusive
    kZeroOrRange,  // 0, or v[0] .. v[1]
    kSet,          // one of v[0 .. 3] (shorter sets repeat their last member)
};
struct OptionRow {
    const char *key;
    int64_t rm_ctx::*member;
    OptionKind kind;
    int64_t v[4];
    const char *error;
};
static const OptionRow kOptions[] = {
    {"tile_w", &rm_ctx::opt_tile_w, kSet, {8, 16, 32, 64}, "tile_w must be 8, 16, 32 or 64"},
    {"filter", &rm_ctx::opt_filter, kSwitch, {}, nullptr},
    {"nodes_in_lds", &rm_ctx::opt_lds, kSwitch, {}, nullptr},
    {"kernel", &rm_ctx::opt_kernel, kRange, {0, 2}, "kernel must be 0 (auto), 1 or 2"},
    {"list_cap", &rm_ctx::opt_list_cap, kRange, {1, 64}, "list_cap must be in [1, 64]"},
    {"coop", &rm_ctx::opt_coop, kSwitch, {}, nullptr},
    {"recs", &rm_ctx::opt_recs, kSwitch, {}, nullptr},
    {"lut", &rm_ctx::opt_lut, kSwitch, {}, nullptr},
    {"uniform", &rm_ctx::opt_uniform, kSwitch, {}, nullptr},
    {"lds_kb", &rm_ctx::opt_lds_kb, kZeroOrRange, {16, 64}, "lds_kb must be 0 (auto) or in [16, 64]"},
    {"multi_step", &rm_ctx::opt_multi_step, kSwitch, {}, nullptr},
    {"step_box", &rm_ctx::opt_step_box, kSwitch, {}, nullptr},
    {"cell_tab", &rm_ctx::opt_cell_tab, kSwitch, {}, nullptr},
    {"runner_up", &rm_ctx::opt_runner_up, kSwitch, {}, nullptr},
    {"item_wide", &rm_ctx::opt_item_wide, kSwitch, {}, nullptr},
    {"prune", &rm_ctx::opt_prune, kSwitch, {}, nullptr},
    {"rtc_spheres", &rm_ctx::opt_rtc_spheres, kRange, {0, 33}, "rtc_spheres must be 0..33"},
    {"specialise_v2_after", &rm_ctx::opt_v2_after, kRange, {0, 1000000}, "specialise_v2_after must be 0 (never) .. 1000000 launches"},
    {"specialise", &rm_ctx::opt_specialise, kRange, {0, 2}, "specialise must be 0, 1 or 2"},
    {"lds_fill", &rm_ctx::opt_lds_fill, kSwitch, {}, nullptr},
    {"min_fill", &rm_ctx::opt_min_fill, kSwitch, {}, nullptr},
    {"overlap_fill", &rm_ctx::opt_overlap_fill, kSwitch, {}, nullptr},
    {"cull", &rm_ctx::opt_cull, kSwitch, {}, nullptr},
    {"rect_cull", &rm_ctx::opt_rect_cull, kSwitch, {}, nullptr},
    {"rel", &rm_ctx::opt_rel, kSwitch, {}, nullptr},
    {"static", &rm_ctx::opt_static, kRange, {0, 95}, "static must be in [0, 95] percent"},  // stored, ignored (rm_ctx)
    {"sub", &rm_ctx::opt_sub, kSwitch, {}, nullptr},
    {"refill", &rm_ctx::opt_refill, kRange, {1, 64}, "refill must be in [1, 64]"},
    {"item_px", &rm_ctx::opt_item_px, kSet, {64, 128, 256, 256}, "item_px must be 64, 128 or 256"},
    {"hw_xcd", &rm_ctx::opt_hw_xcd, kSwitch, {}, nullptr},
    {"grid", &rm_ctx::opt_grid, kSwitch, {}, nullptr},
    {"nn", &rm_ctx::opt_nn, kRange, {0, 2}, "nn must be 0 (off), 1 (on) or 2 (auto)"},
    {"ext", &rm_ctx::opt_ext, kSwitch, {}, nullptr},
    {"blocks_per_cu", &rm_ctx::opt_blocks_per_cu, kRange, {1, 8}, "blocks_per_cu must be in [1, 8]"},
    {"v1_lists", &rm_ctx::opt_v1_lists, kSwitch, {}, nullptr},
    {"v1_block", &rm_ctx::opt_v1_block, kSet, {64, 128, 256, 256}, "v1_block must be 64, 128 or 256"},
    {"oct_lean", &rm_ctx::opt_oct_lean, kSwitch, {}, nullptr},
    {"lpt", &rm_ctx::opt_lpt, kSwitch, {}, nullptr},
    {"n0_batch", &rm_ctx::opt_n0_batch, kRange, {1, 64}, "n0_batch must be in [1, 64]"},
    {"device_build", &rm_ctx::opt_device_build, kSwitch, {}, nullptr},
    {"length", &rm_ctx::opt_length, kRange, {0, 1}, "length must be 0 (Math.hypot) or 1 (Math.sqrt)"},  // part of the numeric contract, not a measurement knob (rm_raymarch.h)
    {"exact", &rm_ctx::opt_exact, kRange, {0, 1}, "exact must be 0 (Scene.getDistance) or 1 (the exact field)"},  // as `length`: selects among defined results
};

static const OptionRow *find_option(const char *key) {
    for (const OptionRow &o : kOptions)
        if (!std::strcmp(key, o.key)) return &o;
    return nullptr;
}

int rm_set_option(rm_ctx *ctx, const char *key, int64_t value) {
    if (!ctx || !key) return RM_E_INVALID;
    const OptionRow *o = find_option(key);
    if (!o) return fail(ctx, RM_E_INVALID, std::string("unknown option ") + key);
    bool ok = true;
    switch (o->kind) {
        case kSwitch: value = value ? 1 : 0; break;
        case kRange: ok = value >= o->v[0] && value <= o->v[1]; break;
        case kZeroOrRange: ok = value == 0 || (value >= o->v[0] && value <= o->v[1]); break;
        case kSet: ok = std::find(std::begin(o->v), std::end(o->v), value) != std::end(o->v); break;
    }
    if (!ok) return fail(ctx, RM_E_INVALID, o->error);
    const bool changed = ctx->*(o->member) != value;
    ctx->*(o->member) = value;
    if (o->member == &rm_ctx::opt_tile_w) ctx->tile_w_set = true;
    if (o->member == &rm_ctx::opt_length && changed && ctx->have_scene) {
        // bounding radii of boxes and smooth unions use vec3.length / vec3.distance too: rebuild the active scene
        ctx->have_scene = false;
        return ensure_scene(ctx, ctx->scene_is_uploaded ? RM_SCENE_UPLOADED : ctx->scene_preset, ctx->host.accel);
    }
    return RM_OK;
}

int rm_get_option(const rm_ctx *ctx, const char *key, int64_t *value) {
    if (!ctx || !key || !value) return RM_E_INVALID;
    const OptionRow *o = find_option(key);
    if (!o) return RM_E_INVALID;
    *value = ctx->*(o->member);
    return RM_OK;
}

}  // extern "C"
