// rm_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the sphere-tracing render path.
//
// One ray per lane.  A 64-lane wavefront owns a tile_w x (64 / tile_w) pixel tile (8 x 8 unless option tile_w says
// otherwise); a workgroup is one wave (option v1_block: up to four tiles stacked vertically) and workgroup ids are dealt
// to tiles in runs of eight per XCD (v1_tile_of_block).  There is no dense contraction
// anywhere on this path, so no MFMA: the work is FP64 VALU (the reference computes in JS
// doubles) with binary32 rounding exactly where the reference stores into Float32Array,
// plus f32 compares for box tests.  Build with -ffp-contract=off: JS never fuses a*b+c.
//
// Reference functions restated here (paths relative to the reference's src/):
//   Raymarcher.runRaymarcher / getSceneDistance / getNormal   cpu_algorithms/raymarcher.ts:46-135
//   SphereTracer.rayMarch                                     cpu_algorithms/sphereTracer.ts:15-83
//   Scene.getDistance                                         util/scene.ts:144-190
//   Primitive.sdf / Sphere.localSdf                           util/primitives/primitive.ts:33-39, sphere.ts:12-14
//   BVH.getPrimitivesAt / findRayIntersections / onRayMarch*  acceleration_structures/bvh.ts:95-240
//   BoundingBox.contains / intersectRay                       acceleration_structures/boundingBox.ts:15-21,69-105
//   Octree.findNode / marchRay / intersectRayBox              acceleration_structures/octree.ts:195-294
//   ShadingModel.shade (4 models)                             util/shading_models/*.ts
//   diagnostics                                               main.ts:528-548
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#include "rm_device.h"

// Diagnostic build only (-DRM_COUNTS, scripts/counts_v1.py): wave-level executions (slot i) and active lanes (slot i + 16)
// per event, straight into P.stamps[8 .. 39] with global atomics (slow; the build exists to count, not to be timed).
#ifdef RM_COUNTS
__device__ unsigned long long *rm_cnt_g;
#define RM_CNT(i)                                                                                  \
    {                                                                                              \
        const unsigned long long n_ = static_cast<unsigned long long>(__popcll(__ballot(1)));      \
        const int l_ = static_cast<int>(__lane_id());                                              \
        if (__builtin_amdgcn_readfirstlane(l_) == l_ && rm_cnt_g) {                                \
            atomicAdd(&rm_cnt_g[8 + (i)], 1ull);                                                   \
            atomicAdd(&rm_cnt_g[8 + (i) + 16], n_);                                                \
        }                                                                                          \
    }
#define RM_CNT1(i) RM_CNT(i)
#else
#define RM_CNT1(i) {}
#endif

#include "rm_bvh_list.h"
#include "rm_program.h"
#ifdef RM_RTC  // the run-time specialiser's build of this file (rm_rtc.cpp): one scene's expression forest as straight-line code
#include "rm_rtc_scene.inc"
#endif
#include "rm_kernels.h"
#include "rm_diag.h"

namespace {

using namespace rmd;

// Fused diagnostics of the one-ray-per-lane kernels (rm_diag.h): a wave stores its 64 pixels once, at its end; the four
// totals of the wave are formed with LDS atomics (lanes outside the frame contribute nothing; eight slots, lane & 7: 64
// lanes on one address would be 64 serial read-modify-writes) and flushed by the wave.  Reached by EVERY lane of every wave
// of the launch (no early return above it), all 64 lanes active.  Out of line, plain arguments: the lean octree kernel
// lives on exactly 64 VGPRs, and inlined this epilogue cost it two spills.
// BLK: the launch's block (RmDiagBlock) or, in a launch of many frames, the block of this workgroup's frame (RmFrameDiagBlock):
// the waves are numbered within blockIdx.x either way -- frames_kernel numbers the frame in blockIdx.y.
template <typename BLK>
__device__ __attribute__((noinline)) static void v1_diag_flush(BLK *blk, RmDiagDevice *out, bool has_pixel, uint32_t c16, uint32_t i16) {
    __shared__ unsigned int v1_diag_s[4][4][8];
    const int lane = static_cast<int>(__lane_id());
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    unsigned int(*w)[8] = v1_diag_s[wave];
    if (lane < 8) w[0][lane] = w[1][lane] = w[2][lane] = w[3][lane] = 0;  // (one wave's LDS operations execute in order)
    if (has_pixel) {
        const int k = lane & 7;
        atomicAdd(&w[0][k], c16);
        atomicAdd(&w[1][k], i16);
        atomicMax(&w[2][k], c16);
        atomicMax(&w[3][k], 0xFFFFFFFFu - c16);
    }
    unsigned int ts = 0, ti = 0, mx = 0, mi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ts += w[0][k];
        ti += w[1][k];
        mx = w[2][k] > mx ? w[2][k] : mx;
        mi = w[3][k] > mi ? w[3][k] : mi;
    }
    const unsigned int wpw = blockDim.x >> 6;
    diag_flush_wave<true>(blk, out, nullptr, ts, ti, mx, mi, blockIdx.x * wpw + static_cast<unsigned int>(wave), gridDim.x * wpw, lane);
}
template <typename BLK>
__device__ __forceinline__ void v1_diag_epilogue(BLK *blk, RmDiagDevice *out, bool has_pixel, uint32_t c16, uint32_t i16) {
    if (blk) v1_diag_flush(blk, out, has_pixel, c16, i16);
}

// ------------------------------------------------------------------ Scene.getDistance

// min over a primitive list for either scene representation
// GEN is a compile-time property of the kernel instantiation: a run-time `if (P.general)` in
// front of the sphere loop changed the results of render_kernel<0, true> (lane-grouping
// dependent wrong normals with hipcc 7.2), so the two representations never share a function body.
// GEN: 0 RmSphere records, 1 RmPrim records, 2 expression programs (rm_program.h), 3 programs with a Mandelbulb,
// 4 (RM_RTC builds only) the scene's programs as generated straight-line code.
template <int GEN>
__device__ __forceinline__ double list_min(const RmRenderParams &P, const int32_t *ids, int n, const Vec3f &p,
                                           double closest) {
#ifdef RM_RTC
    if (GEN == 4) {  // the scene's own code (generated: rm_rtc.cpp); per-lane object ids, no instruction stream
        for (int k = 0; k < n; ++k) closest = js_min_nan(rm_rtc_object_sdf(ids ? ids[k] : k, p, P.time), closest);
        return closest;
    }
#endif
    if (GEN >= 2) {  // Math.min(primitive.sdf(position), closestDistance), NaN-propagating
        for (int k = 0; k < n; ++k) {
            const int obj = ids ? ids[k] : k;
            // The interpreter reads its instruction stream through the scalar cache, so it runs ONE object at a time: lanes whose
            // lists name different objects at this position (different leaves) take turns (a waterfall over the distinct ids).
            double d = 0.0;
            for (bool done = false; !done;) {
                const int u = __builtin_amdgcn_readfirstlane(obj);
                if (obj == u) {
                    d = program_sdf<GEN == 3>(P.prog, P.obj_ranges[2 * u], P.obj_ranges[2 * u + 1], p, P.time, P.prog_slots);
                    done = true;
                }
            }
            closest = js_min_nan(d, closest);
        }
        return closest;
    }
    if (GEN == 1) {
        for (int k = 0; k < n; ++k) closest = min_dist(prim_sdf_general(P.prims[ids ? ids[k] : k], p), closest);
        return closest;
    }
#ifdef RM_REPRO_GENERAL_BRANCH  // round 1's form: the representation chosen by a RUN-TIME branch in the sphere instantiation
    if (P.general) {
        for (int k = 0; k < n; ++k) closest = min_dist(prim_sdf_general(P.prims[ids ? ids[k] : k], p), closest);
        return closest;
    }
#endif
    if (P.filter && n >= 2) return prims_min_best<int32_t>(P.spheres, P.radii, ids, n, 0, p, closest);  // scan, then one exact evaluation
    return prims_min<true>(P.spheres, P.radii, ids, n, p, closest, false);  // shared-reciprocal Math.hypot (bit-identical: rm_selftest_fastdiv)
}

// scene.ts:183-189 and the BVH fallback scene.ts:173: every primitive, all counted
// General primitives: the reference evaluates all N (scene.ts:173,183-189); with rigid transforms every primitive has a
// bounding sphere (centre c, radius R; host: build_scene_general) with |p - c| - R <= sdf(p) <= |p - c| + R, so a primitive
// whose lower bound exceeds the smallest upper bound (or 10, the starting value of `closest`) cannot attain
// min(10, min_j sdf_j(p)).  Binary32 bounds with the same error margin as the spheres' filter (sphere_sdf_estimate); only
// the survivors -- a handful of 40 -- are evaluated exactly (transformMat4 + Box / Torus / Sphere localSdf in binary64).
// Math.min is order independent, so the value is bit-identical; all N are counted.
__device__ double general_prims_filtered(const RmRenderParams &P, const Vec3f &p) {
    float ub = 10.0f;
    for (int j = 0; j < P.n_prims; ++j) {
        const RmSphere b = P.spheres[j];
        const float dx = p.x - b.cx, dy = p.y - b.cy, dz = p.z - b.cz;
        const float len = __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz);
        const float hi = (len + b.rf) + (len + b.rf + 1.0f) * 4e-6f;
        ub = hi < ub ? hi : ub;
    }
    double closest = RM_MAX_DIST;
    for (int j = 0; j < P.n_prims; ++j) {
        const RmSphere b = P.spheres[j];
        const float dx = p.x - b.cx, dy = p.y - b.cy, dz = p.z - b.cz;
        const float len = __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz);
        const float lo = (len - b.rf) - (len + b.rf + 1.0f) * 4e-6f;
        if (lo <= ub) closest = min_dist(prim_sdf_general(P.prims[j], p), closest);
    }
    return closest;
}

template <int GEN>
__device__ double all_prims_distance(const RmRenderParams &P, const Vec3f &p, uint32_t &count) {
    double closest = RM_MAX_DIST;
    if (GEN == 1 && P.prim_filter && P.n_prims >= 8) closest = general_prims_filtered(P, p);
    else closest = list_min<GEN>(P, nullptr, P.n_prims, p, closest);
    count += static_cast<uint32_t>(P.n_prims);
    return closest;
}

// scene.ts:167-181 with BVH.getPrimitivesAt (bvh.ts:95-121): union of the primitives of
// every leaf whose box contains p (a primitive lives in exactly one leaf), else all.
template <int GEN>
__device__ double bvh_distance(const RmRenderParams &P, const Vec3f &p, uint32_t &count) {
#ifdef RM_RTC_BVH_LEAVES  // this scene's leaves are code (rm_rtc.cpp, emit_bvh): no node loads, the objects called by name
    if (GEN == 4) return rm_rtc_bvh_distance(p, P.time, count);
#endif
    double closest = RM_MAX_DIST;
    uint32_t found = 0;
    int i = 0;
    int n = P.bvh_nodes;
    if (GEN < 2 && P.use_grid) {  // (not for expression programs: few objects, and their kernels are at the register limit)
        // BVH.getPrimitivesAt through the leaf grid (rm_scene_host.cpp build_point_query_grid): the leaves listed for p's
        // cell are a superset of the leaves whose box contains p; each is re-tested with the reference's inclusive
        // binary32 compares, and outside the root box no leaf can contain p.  Crowded cells keep the tree walk.
        const RmBvhNode root = P.bvh[0];
        bool walk = false;
        if (box_contains(root.lo, root.hi, p)) {
            const int cx = min(max(static_cast<int>((p.x - P.pq_origin[0]) * P.pq_inv[0]), 0), P.pq_dim[0] - 1);
            const int cy = min(max(static_cast<int>((p.y - P.pq_origin[1]) * P.pq_inv[1]), 0), P.pq_dim[1] - 1);
            const int cz = min(max(static_cast<int>((p.z - P.pq_origin[2]) * P.pq_inv[2]), 0), P.pq_dim[2] - 1);
            const uint32_t cell = P.pq_cells[(cz * P.pq_dim[1] + cy) * P.pq_dim[0] + cx];
            const int ccnt = static_cast<int>(cell & 0xFFu);
            if (ccnt == 255) walk = true;
            else {
                const uint16_t *lst = P.pq_list + (cell >> 8);
                for (int e = 0; e < ccnt; ++e) {
                    const RmBvhNode node = P.bvh[lst[e]];
                    if (!box_contains(node.lo, node.hi, p)) continue;
                    const int first = node.leaf >> 8, cnt = node.leaf & 0xFF;
                    closest = list_min<GEN>(P, P.bvh_prims + first, cnt, p, closest);
                    found += static_cast<uint32_t>(cnt);
                }
            }
        }
        if (!walk) n = 0;  // the grid answered: skip the walk
    }
    while (i < n) {
        const RmBvhNode node = P.bvh[i];
        if (!box_contains(node.lo, node.hi, p)) {
            i = node.skip;
            continue;
        }
        if (node.leaf < 0) {
            i = i + 1;
            continue;
        }
        const int first = node.leaf >> 8, cnt = node.leaf & 0xFF;
        closest = list_min<GEN>(P, P.bvh_prims + first, cnt, p, closest);
        found += static_cast<uint32_t>(cnt);
        i = node.skip;
    }
    if (found == 0) return all_prims_distance<GEN>(P, p, count);
    count += found;
    return closest;
}

// Octree.findNode (octree.ts:223-248): -1 when p is outside the root cube.  Children tile
// their parent at the f32 centre and `contains` is inclusive, so the first child (index
// order x + 2y + 4z) that contains p takes the low half on every axis where p <= centre.
// With the cell table: on each axis the leaf is the cell k with b_k < p <= b_{k+1} (b_k = -10 + 0.3125 k,
// exact in binary32; the lowest cell also takes p = -10), which is what "first child that contains p" selects.
// k is guessed from a binary32 product (off by at most one cell) and corrected with exact compares.
__device__ __forceinline__ int oct_cell(float v) {
    int k = static_cast<int>((v + 10.0f) * 3.2f);
    k = k < 0 ? 0 : (k > 63 ? 63 : k);
    const float b = -10.0f + 0.3125f * static_cast<float>(k);  // exact
    if (v <= b && k > 0) k -= 1;
    else if (v > b + 0.3125f && k < 63) k += 1;
    return k;
}

__device__ int oct_find(const RmRenderParams &P, const Vec3f &p) {
    const RmOctNode *nodes = P.oct;
    if (!box_contains(nodes[0].lo, nodes[0].hi, p)) return -1;
    if (P.oct_lut) return P.oct_lut[(oct_cell(p.z) * 64 + oct_cell(p.y)) * 64 + oct_cell(p.x)];
    int i = 0;
    for (;;) {
        const int first = nodes[i].first_child;
        if (first < 0) return i;
        const float cx = nodes[i].center[0], cy = nodes[i].center[1], cz = nodes[i].center[2];
        i = first + (p.x > cx ? 1 : 0) + (p.y > cy ? 2 : 0) + (p.z > cz ? 4 : 0);
    }
}

// One leaf-ordered record against the running minimum (same filter as prims_min)
__device__ __forceinline__ void rec_consider(const float4 c, const RmSphereRec *rec, const Vec3f &p, double &closest, float &ub) {
    const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
    const float len = __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz);
    const float err = (len + __builtin_fabsf(c.w) + 1.0f) * 4e-6f;  // sphere_sdf_estimate
    if ((len - c.w) - err <= ub) {
        const double e = vec3_length(dx, dy, dz) - rec->radius;
        if (e < closest) {
            closest = e;
            ub = f32_upper_bound(e);
        }
    }
}

// min over a leaf's sphere records (RmSphereRec).  Lanes of a wave sit in different leaves, so a loop that
// evaluates a sphere exactly as soon as its bound passes runs the 40-instruction FP64 body once per distinct
// position at which SOME lane passes -- measured ~9 times per leaf visit on the 10k-sphere scene, each for a few
// lanes.  Instead the scan only keeps, per lane, the sphere with the smallest upper bound (k1, hi1, lb1) and the
// smallest lower bound among all the others (lb2); afterwards every lane evaluates its k1 exactly in the SAME
// instruction stream.  If lb2 exceeds that exact value no other sphere can be closer (exact_j >= lb_j >= lb2);
// otherwise (near ties) the list is rescanned with the ordinary filter.  Four 16-B loads are in flight per step.
// `sub` != nullptr: only the listed positions are scanned (the sub-cell's candidates, rm_scene_host.h); the near-tie
// rescan always covers the whole list.
__device__ double recs_min(const RmSphereRec *recs, int n, const Vec3f &p, double closest, const uint8_t *sub = nullptr,
                           int n_sub = 0) {
    if (n <= 0) return closest;
    const float inf = __builtin_inff();
    int k1 = 0;
    float hi1 = inf, lb1 = inf, lb2 = inf;
    auto scan = [&](const float4 c, int k) {
        const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
        const float len = __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz);
        const float err = (len + __builtin_fabsf(c.w) + 1.0f) * 4e-6f;  // sphere_sdf_estimate
        const float a = len - c.w, lb = a - err, hi = a + err;
        const bool better = hi < hi1;
        lb2 = __builtin_fminf(lb2, better ? lb1 : lb);
        k1 = better ? k : k1;
        lb1 = better ? lb : lb1;
        hi1 = better ? hi : hi1;
    };
    int k = 0;
    if (sub) {
        for (int e = 0; e < n_sub; ++e) {
            RM_CNT1(6)
            const int j = sub[e];
            scan(*reinterpret_cast<const float4 *>(recs + j), j);
        }
        k = n;  // skip the full scan below
    }
    for (; k + 4 <= n; k += 4) {
        RM_CNT1(7)
        const float4 c0 = *reinterpret_cast<const float4 *>(recs + k);
        const float4 c1 = *reinterpret_cast<const float4 *>(recs + k + 1);
        const float4 c2 = *reinterpret_cast<const float4 *>(recs + k + 2);
        const float4 c3 = *reinterpret_cast<const float4 *>(recs + k + 3);
        scan(c0, k);
        scan(c1, k + 1);
        scan(c2, k + 2);
        scan(c3, k + 3);
    }
    for (; k < n; ++k) {
        RM_CNT1(15)
        scan(*reinterpret_cast<const float4 *>(recs + k), k);
    }
    {
        RM_CNT1(8)
        const float4 c = *reinterpret_cast<const float4 *>(recs + k1);
        const double e = vec3_length(p.x - c.x, p.y - c.y, p.z - c.z) - recs[k1].radius;
        closest = e < closest ? e : closest;
    }
    float ub = f32_upper_bound(closest);
    if (lb2 <= ub) {  // another sphere may tie or win: ordinary filtered pass over the whole list
        RM_CNT1(9)
        for (k = 0; k < n; ++k) rec_consider(*reinterpret_cast<const float4 *>(recs + k), recs + k, p, closest, ub);
    }
    return closest;
}

// scene.ts:148-166 given the node findNode returned
template <int GEN>
__device__ double oct_node_distance(const RmRenderParams &P, int node, const Vec3f &p, uint32_t &count) {
    if (node < 0) {
        RM_CNT1(12)
        return all_prims_distance<GEN>(P, p, count);  // outside the cube: scene.ts:166,183-189
    }
    const RmOctNode nd = P.oct[node];
    double closest = RM_MAX_DIST;
    if (nd.prim_count > 0) {
        RM_CNT1(2)
        if (GEN == 0 && P.oct_recs && P.filter) {
            const uint8_t *sub = nullptr;
            int n_sub = 0;
            if (P.oct_sub_hdr && nd.sub_first >= 0) {  // crowded leaf: the candidates of p's sub-cell
                const float ix = nd.center[0], iy = nd.center[1], iz = nd.center[2];  // RM_OCT_SUB / (hi - lo), from the host
                const int sx = min(max(static_cast<int>((p.x - nd.lo[0]) * ix), 0), RM_OCT_SUB - 1);
                const int sy = min(max(static_cast<int>((p.y - nd.lo[1]) * iy), 0), RM_OCT_SUB - 1);
                const int sz = min(max(static_cast<int>((p.z - nd.lo[2]) * iz), 0), RM_OCT_SUB - 1);
                const uint32_t hdr = P.oct_sub_hdr[nd.sub_first + (sz * RM_OCT_SUB + sy) * RM_OCT_SUB + sx];
                sub = P.oct_sub_list + (hdr >> 8);
                n_sub = static_cast<int>(hdr & 0xFFu);
            }
            closest = recs_min(P.oct_recs + nd.prim_first, nd.prim_count, p, closest, sub, n_sub);
        }
        else closest = list_min<GEN>(P, P.oct_prims + nd.prim_first, nd.prim_count, p, closest);
        count += static_cast<uint32_t>(nd.prim_count);
    } else if (nd.is_empty) {
        RM_CNT1(11)
        closest = min_dist(nd.min_distance * 0.99, closest);  // Math.min(closest, minDistance * safety)
    }
    return closest;
}

// ACCEL 3 (option `exact`; point, field and tile queries only): the exact field, defined with the sparse mesher below
template <int GEN>
__device__ double exact_distance(const RmRenderParams &P, const Vec3f &p, uint32_t &count);

template <int ACCEL, int GEN>
__device__ __forceinline__ double scene_distance(const RmRenderParams &P, const Vec3f &p, uint32_t &count) {
    if constexpr (ACCEL == 3) return exact_distance<GEN>(P, p, count);
    if (ACCEL == 2) return bvh_distance<GEN>(P, p, count);
    if (ACCEL == 1) return oct_node_distance<GEN>(P, oct_find(P, p), p, count);
    return all_prims_distance<GEN>(P, p, count);
}

// ------------------------------------------------------------------ BVH ray intervals

// The reference materialises every leaf interval of the ray, stable-sorts them by tEnter
// (bvh.ts:126-178) and walks the list with an index (bvh.ts:204-240).  This returns the
// element that follows key (keyT, keyOrd) in exactly that order -- ascending tEnter, ties
// in traversal order -- by one stackless traversal, so no per-ray list is stored.
__device__ bool bvh_next_interval(const RmRenderParams &P, const Ray &r, const RayInv &ri, double keyT, int keyOrd,
                                  Interval &out) {
#ifdef RM_RTC_BVH_LEAVES
    return rm_rtc_bvh_next_interval(r, ri, keyT, keyOrd, out);
#else
    bool have = false;
    int i = 0;
    const int n = P.bvh_nodes;
    while (i < n) {
        const RmBvhNode node = P.bvh[i];
        double tE, tX;
        // 1 / direction[i] (boundingBox.ts:78) is the same quotient for every box: computed once per ray
        if (!slab_inv(node.lo, node.hi, r, ri, tE, tX) || tX < 0.0 || tE > RM_MAX_DIST) {  // bvh.ts:145,151
            i = node.skip;
            continue;
        }
        if (node.leaf < 0) {
            i = i + 1;
            continue;
        }
        if ((node.leaf & 0xFF) > 0) {  // bvh.ts:165
            const double cE = tE > 0.0 ? tE : 0.0;                  // Math.max(tEnter, tMin = 0)
            const double cX = tX < RM_MAX_DIST ? tX : RM_MAX_DIST;  // Math.min(tExit, tMax = 10)
            const bool after = cE > keyT || (cE == keyT && i > keyOrd);
            const bool better = !have || cE < out.tEnter;  // equal tEnter: earlier node wins, seen first
            if (after && better) {
                out.tEnter = cE;
                out.tExit = cX;
                out.ord = i;
                have = true;
            }
        }
        i = node.skip;
    }
    return have;
#endif
}

// ------------------------------------------------------------------ the render kernel

// raymarcher.ts:123-135 getNormal at `hit`, its first evaluation -- Scene.getDistance(hit) -- handed in as d0: the three
// offset evaluations are added to count.  hit_normal's arithmetic, and G(p, d) of the point queries (point_kernel).
template <int ACCEL, int GEN>
__device__ __forceinline__ Vec3f distance_gradient(const RmRenderParams &P, const Vec3f &hit, double d0, uint32_t &count) {
    float nx, ny, nz;
    Vec3f q = hit;
    q.x = to_f32(static_cast<double>(hit.x) - 0.01);
    nx = to_f32(d0 - scene_distance<ACCEL, GEN>(P, q, count));
    q = hit;
    q.y = to_f32(static_cast<double>(hit.y) - 0.01);
    ny = to_f32(d0 - scene_distance<ACCEL, GEN>(P, q, count));
    q = hit;
    q.z = to_f32(static_cast<double>(hit.z) - 0.01);
    nz = to_f32(d0 - scene_distance<ACCEL, GEN>(P, q, count));
    double len = static_cast<double>(nx) * nx + static_cast<double>(ny) * ny + static_cast<double>(nz) * nz;
    if (len > 0) len = 1 / __builtin_sqrt(len);
    nx = to_f32(nx * len);
    ny = to_f32(ny * len);
    nz = to_f32(nz * len);
    return Vec3f{nx, ny, nz};
}

// raymarcher.ts:94-102: the normal at hitPosition = f32(o + d * depth), (0, 0, 0) when depth >= MAX_DIST; getNormal's four
// evaluations are added to count.  Shared by the render kernels (normal_and_store) and the ray queries (cast_kernel).
template <int ACCEL, int GEN>
__device__ __forceinline__ Vec3f hit_normal(const RmRenderParams &P, const Ray &ray, double depth, uint32_t &count) {
    Vec3f hit;
    hit.x = to_f32(static_cast<double>(ray.o.x) + static_cast<double>(ray.d.x) * depth);
    hit.y = to_f32(static_cast<double>(ray.o.y) + static_cast<double>(ray.d.y) * depth);
    hit.z = to_f32(static_cast<double>(ray.o.z) + static_cast<double>(ray.d.z) * depth);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (!(depth >= RM_MAX_DIST)) {
        RM_CNT1(13)
        const double d0 = scene_distance<ACCEL, GEN>(P, hit, count);
        const Vec3f n = distance_gradient<ACCEL, GEN>(P, hit, d0, count);
        nx = n.x;
        ny = n.y;
        nz = n.z;
    }
    return Vec3f{nx, ny, nz};
}

template <int ACCEL, int GEN>
__device__ double normal_and_store(const RmRenderParams &P, const Ray &ray, double depth, uint32_t &count,
                                   uint8_t nb[3]) {
    // raymarcher.ts:94-105
    const Vec3f n = hit_normal<ACCEL, GEN>(P, ray, depth, count);
    nb[0] = u8clamp((static_cast<double>(n.x) + 1) * 0.5 * 255);
    nb[1] = u8clamp((static_cast<double>(n.y) + 1) * 0.5 * 255);
    nb[2] = u8clamp((static_cast<double>(n.z) + 1) * 0.5 * 255);
    return depth;
}

// The per-ray hit-leaf list of rm_bvh_list.h in this kernel: BVH.onRayMarchStart walks the tree once and records the
// leaves the ray hits; every later "next interval" scans that short list instead of walking the whole tree again with a
// slab test per node (what bvh_next_interval does; it remains for launches without the list).  The list lives in dynamic
// LDS behind the expression programs' slots (list_lds_offset), RM_V1_LIST_CAP entries of 2 B per lane.
#define RM_V1_LIST_CAP 16
__device__ __forceinline__ SceneView v1_view(const RmRenderParams &P) {
    SceneView S;
    S.nodes = P.bvh;
    S.bvh_prims = P.bvh_prims;
    S.oct = P.oct;
    S.oct_prims = P.oct_prims;
    S.spheres = P.spheres;
    S.radii = P.radii;
    S.pq_cells = P.pq_cells;
    S.pq_list = P.pq_list;
    S.nn_cells = P.nn_cells;
    S.nn_list = P.nn_list;
    S.ext_cells = nullptr;  // (the one-ray-per-lane kernels do not use the exterior candidate grid)
    S.ext_list = nullptr;
    S.rel = nullptr;
    S.n_prims = P.n_prims;
    S.bvh_nodes = P.bvh_nodes;
    return S;
}
__device__ __forceinline__ RayList v1_ray_list(const RmRenderParams &P) {
    extern __shared__ __align__(16) unsigned char v1_smem[];
    RayList L;
    L.cap = RM_V1_LIST_CAP;
    L.cnt = L.live = L.cur_pos = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    L.col = reinterpret_cast<uint16_t *>(v1_smem + P.v1_list_offset) + (static_cast<size_t>(wave) * RM_V1_LIST_CAP) * 64 + lane;
    return L;
}

// What a marcher tells about its walk (rm_ray_walk, include/rm_raymarch.h): eval at every Scene.getDistance call that adds to
// iters (t: the parameter the point was formed at; n: the primitives that call counted), skip at every positive answer of
// the acceleration structure (t: the parameter before it), end at every exit but the exhausted trip limit (a recorder
// starts at RM_WALK_STEPS).  The recorder is a parameter pack of none or one: renders and the other ray queries pass none, and
// their marchers keep the signature and the body they had -- every hook below is a fold over an empty pack, no code at all
// (a defaulted no-op recorder argument was tried: it moved SGPR spills and two VGPRs in some GEN 2 / 3 instantiations).
enum { RM_WALK_HIT = 0, RM_WALK_FAR = 1, RM_WALK_STEPS = 2, RM_WALK_ACCEL = 3 };  // rm_walk_end
#define RM_REC(call) ((void)(rec.call), ...)

// SphereTracer.rayMarch (sphereTracer.ts:15-83)
template <int ACCEL, int GEN, typename... REC>
__device__ double ray_march(const RmRenderParams &P, const Ray &ray, uint32_t &count, uint32_t &iters, REC &...rec) {
    double t = 0.0;
    Interval cur;
    bool haveCur = false;
    RayInv ri;
    OctInv oinv;
    RayList L;
    const bool lists = ACCEL == 2 && GEN < 2 && P.v1_list_offset >= 0;  // expression programs: a handful of objects, nothing to gain
    if (ACCEL == 1) oinv = make_oct_inv(ray);
    if (ACCEL == 2) {
        ri = make_ray_inv(ray);
        if (lists) {
            L = v1_ray_list(P);
            haveCur = bvh_prologue<false>(v1_view(P), ray, ri, L, cur);  // onRayMarchStart
        } else {
            haveCur = bvh_next_interval(P, ray, ri, -__builtin_inf(), -1, cur);
        }
        if (!haveCur) {  // bvh.ts:190-192
            RM_REC(end(RM_WALK_ACCEL));
            return RM_MAX_DIST;
        }
    }
    for (int i = 0; i < RM_MAX_STEPS; ++i) {
        RM_CNT1(0)
        Vec3f p;
        p.x = to_f32(static_cast<double>(ray.o.x) + static_cast<double>(ray.d.x) * t);
        p.y = to_f32(static_cast<double>(ray.o.y) + static_cast<double>(ray.d.y) * t);
        p.z = to_f32(static_cast<double>(ray.o.z) + static_cast<double>(ray.d.z) * t);
        int onode = -1;
        if (ACCEL == 2) {
            // BVH.onRayMarchStep (bvh.ts:204-240)
            double skip = 0.0;
            if (!haveCur) {  // currentIntervalIdx >= length
                RM_REC(end(RM_WALK_ACCEL));
                return RM_MAX_DIST;
            }
            if (t < cur.tEnter) skip = cur.tEnter - t;
            else if (t > cur.tExit) {
                const Interval prev = cur;
                haveCur = lists ? bvh_next<false>(v1_view(P), ray, ri, L, prev.tEnter, prev.ord, cur)
                                : bvh_next_interval(P, ray, ri, prev.tEnter, prev.ord, cur);  // idx++
                if (!haveCur) {
                    RM_REC(end(RM_WALK_ACCEL));
                    return RM_MAX_DIST;
                }
                if (cur.tEnter > t) skip = cur.tEnter - t;
            }
            if (skip > 0.0) {
                RM_REC(skip(t, skip));
                t += skip;
                if (t > RM_MAX_DIST) {
                    RM_REC(end(RM_WALK_FAR));
                    break;
                }
                continue;
            }
        } else if (ACCEL == 1) {
            onode = oct_find(P, p);  // marchRay recomputes this same point
            if (onode >= 0) {
                const double skip = oct_skip(P.oct[onode], ray, t, oinv);
                if (skip > 0.0) {
                    RM_CNT1(1)
                    RM_REC(skip(t, skip));
                    t += skip;
                    if (t > RM_MAX_DIST) {
                        RM_REC(end(RM_WALK_FAR));
                        break;
                    }
                    continue;
                }
            }
        }
        [[maybe_unused]] const uint32_t before = count;
        double dist;
        if (ACCEL == 1) dist = oct_node_distance<GEN>(P, onode, p, count);
        else dist = scene_distance<ACCEL, GEN>(P, p, count);
        RM_REC(eval(t, dist, count - before));
        t += dist;
        iters += 1;
        if (dist < RM_EPSILON) {
            RM_REC(end(RM_WALK_HIT));
            break;
        }
        if (t > RM_MAX_DIST) {
            RM_REC(end(RM_WALK_FAR));
            break;
        }
    }
    return t;
}

// The four other marchers of the Algorithm plugin (raymarchWorker.ts:49-68) share the accel
// prologue and skip protocol of the sphere tracer and differ in the step rule:
//   1 FixedStep       fixedStep.ts:21-94        MAX_STEPS 200, returns MAX_DIST unless it hit
//   2 AdaptiveStep    adaptiveStep.ts:22-105    MAX_STEPS 200, step = clamp(0.8 d, 0.025, 0.5) or 0.01 near
//   3 AdaptiveStepV2  adaptiveStepV2.ts:22-124  overshoot by overshootFactor, step back when spheres do not overlap
//   4 AdaptiveStepV3  adaptiveStepV3.ts:22-137  as V2 plus the "bridging" third evaluation
template <int ACCEL, int GEN, typename... REC>
__device__ double ray_march_other(const RmRenderParams &P, const Ray &ray, uint32_t &count, uint32_t &iters, REC &...rec) {
    const int alg = P.algorithm;
    const int max_steps = (alg == 1 || alg == 2) ? 200 : 100;
    const double FIXED_STEP_SIZE = 0.1, STEP_SCALE = 0.8;
    const double MIN_STEP = FIXED_STEP_SIZE * 0.25, MAX_STEP = FIXED_STEP_SIZE * 5.0;
    const double NEAR_DIST = 0.1, NEAR_STEP = 0.01;
    double t = 0.0, prevSDF = 0.0, prevStep = 0.0;
    bool hit = false;
    Interval cur;
    bool haveCur = false;
    RayInv ri;
    OctInv oinv;
    RayList L;
    const bool lists = ACCEL == 2 && GEN < 2 && P.v1_list_offset >= 0;  // expression programs: a handful of objects, nothing to gain
    if (ACCEL == 1) oinv = make_oct_inv(ray);
    if (ACCEL == 2) {
        ri = make_ray_inv(ray);
        if (lists) {
            L = v1_ray_list(P);
            haveCur = bvh_prologue<false>(v1_view(P), ray, ri, L, cur);
        } else {
            haveCur = bvh_next_interval(P, ray, ri, -__builtin_inf(), -1, cur);
        }
        if (!haveCur) {
            RM_REC(end(RM_WALK_ACCEL));
            return RM_MAX_DIST;
        }
    }
    for (int i = 0; i < max_steps; ++i) {
        Vec3f p = point_at(ray, t);
        int onode = -1;
        double skip = 0.0;
        if (ACCEL == 2) {  // BVH.onRayMarchStep (bvh.ts:204-240)
            if (!haveCur) {
                RM_REC(end(RM_WALK_ACCEL));
                return RM_MAX_DIST;
            }
            if (t < cur.tEnter) skip = cur.tEnter - t;
            else if (t > cur.tExit) {
                const Interval prev = cur;
                haveCur = lists ? bvh_next<false>(v1_view(P), ray, ri, L, prev.tEnter, prev.ord, cur)
                                : bvh_next_interval(P, ray, ri, prev.tEnter, prev.ord, cur);
                if (!haveCur) {
                    RM_REC(end(RM_WALK_ACCEL));
                    return RM_MAX_DIST;
                }
                if (cur.tEnter > t) skip = cur.tEnter - t;
            }
        } else if (ACCEL == 1) {
            onode = oct_find(P, p);
            if (onode >= 0) skip = oct_skip(P.oct[onode], ray, t, oinv);
        }
        if (skip > 0.0) {
            RM_REC(skip(t, skip));
            t += skip;
            if (t > RM_MAX_DIST) {
                RM_REC(end(RM_WALK_FAR));
                break;
            }
            prevSDF = 0.0;  // adaptiveStepV2.ts:73-74 (harmless for the marchers without this state)
            prevStep = 0.0;
            continue;
        }
        [[maybe_unused]] const uint32_t before = count;
        const double dist = ACCEL == 1 ? oct_node_distance<GEN>(P, onode, p, count) : scene_distance<ACCEL, GEN>(P, p, count);
        RM_REC(eval(t, dist, count - before));
        iters += 1;
        if (alg == 1 || alg == 2) {
            if (dist < RM_EPSILON) {
                RM_REC(end(RM_WALK_HIT));
                hit = true;
                break;
            }
            double step;
            if (alg == 1) step = P.step_size;
            else if (dist < NEAR_DIST) step = NEAR_STEP;
            else {
                step = STEP_SCALE * dist;
                if (step < MIN_STEP) step = MIN_STEP;
                if (step > MAX_STEP) step = MAX_STEP;
            }
            t += step;
            if (t > RM_MAX_DIST) {
                RM_REC(end(RM_WALK_FAR));
                break;
            }
            continue;
        }
        // AdaptiveStepV2 / V3
        if (dist < RM_EPSILON) {
            RM_REC(end(RM_WALK_HIT));
            break;
        }
        if (t > RM_MAX_DIST) {
            RM_REC(end(RM_WALK_FAR));
            break;
        }
        if (i == 0 || prevSDF == 0.0) {
            t += dist;
            prevSDF = dist;
            prevStep = dist;
            continue;
        }
        if (prevStep <= (prevSDF + dist)) {  // spheresOverlapped
            const double step = dist * P.overshoot;
            t += step;
            prevSDF = dist;
            prevStep = step;
            continue;
        }
        if (alg == 3) {  // adaptiveStepV2.ts:108-114
            t -= prevStep;
            t += prevSDF;
            prevStep = prevSDF;
            continue;
        }
        // adaptiveStepV3.ts:103-130
        const double originalPos = t - prevStep;
        t = originalPos + prevSDF;
        p = point_at(ray, t);
        [[maybe_unused]] const uint32_t before3 = count;
        const double d3 = scene_distance<ACCEL, GEN>(P, p, count);
        RM_REC(eval(t, d3, count - before3));
        iters += 1;
        if (prevSDF + dist + d3 >= prevStep) {
            t = originalPos + prevStep + dist;
            prevSDF = dist;
            prevStep = dist;
            continue;
        }
        prevSDF = d3;
        prevStep = d3;
        t += d3;
    }
    if (alg == 1 || alg == 2) return hit ? t : RM_MAX_DIST;
    return t;
}

#undef RM_REC

// Workgroup id -> tile for the one-ray-per-lane kernels.  Workgroups go to the eight XCDs round-robin (id % 8), each with
// its own L2; a wave tile is 8 pixels wide, so a tile row writes 32-byte pieces of 128-byte lines.  Tiles are therefore
// dealt in runs of eight: ids 0, 8, 16 ... 56 (all on XCD 0, back to back) are tiles 0 ... 7, ids 1, 9, ... are tiles
// 8 ... 15, and so on: the pieces of a line meet in one L2 and leave as whole lines.  (The launcher rounds the grid up to
// a multiple of 64; ids past the last tile return.)
__device__ __forceinline__ int v1_tile_of_block(int b) {
    const int r = b & 63;
    return (b & ~63) + ((r & 7) << 3) + (r >> 3);
}

#ifndef RM_RTC  // (the lean octree kernel serves sphere scenes only)
// ------------------------------------------------------------------ the octree sphere tracer, lean form
//
// render_kernel<1, false, 0> spends 60 % of its instructions in the part of the march step that precedes the distance
// (scripts/counts_v1.py on the 10 000-sphere scene: 61 loop trips per wave, 38 of them end in a skip; ~135 VALU
// instructions per trip for findNode + marchRay, and ten dependent loads in a row).  The same arithmetic with less
// around it, for sphere scenes whose octree has the cell table (the launcher checks: rm_launch_render):
//  * findNode: the root cube is [-10, 10]^3 (scene.ts:81-85), so `contains` is max(|x|, |y|, |z|) <= 10 (the march
//    point is finite: finite camera, finite t); the cell index is guessed from a product that is biased UPWARDS
//    (3.20001f: never below the true cell, at most one above -- |error| of the two binary32 roundings and of the
//    constant < 4e-6 relative, cells <= 64) and corrected with ONE exact compare against the cell's lower face
//    (b_k = -10 + 0.3125 k, exact in binary32, formed with an fma that therefore rounds nothing).
//  * marchRay / intersectRayBox (octree.ts:195-220,250-294): the reference swaps t0 / t1 when 1 / d < 0; here the ray
//    knows from its direction signs which face is the far and which the near one on every axis and loads them with
//    per-lane byte offsets: no selects, same products.  The comparisons of the binary32 tMin / tMax are made in
//    binary32 (exact either way) and without branches.
//  * every load is base (SGPR pair) + 32-bit byte offset, and everything a step can need from the node record is
//    requested in ONE batch right after the cell table's answer.
//  * (face - origin) is the same binary64 difference for every ray of a frame: oct_frame_table_kernel forms it once per
//    node and camera position (RmOctFrameNode; rm_api.cpp keeps the tables of the last few camera positions), and the
//    march step multiplies it by the ray's 1 / d.  minDistance * 0.99 (octree.ts:282) sits beside it.
//  * getNormal's four samples are four more trips of the SAME loop (a phase per ray, as in the v2 kernel): one copy of
//    the distance code, and a ray that has finished marching shares its evaluations with neighbours that still march.
// Leaf records, sub-cell candidate lists, filter margins, shading and counters are those of render_kernel<1, ...>,
// which stays the independent cross-check (option `oct_lean` = 0).
__device__ __forceinline__ uint32_t oct_cell_up(float v) {
    const float g = __builtin_truncf((v + 10.0f) * 3.20001f);          // in [0, 64]
    const float b = __builtin_fmaf(g, 0.3125f, -10.0f);                // exact: lower face of cell g
    const int k = static_cast<int>(g) - (v <= b ? 1 : 0);              // the lowest cell also takes v = -10 (clamp)
    return static_cast<uint32_t>(min(max(k, 0), 63));
}

template <typename T>
__device__ __forceinline__ T ld_off(const void *base, uint32_t byte_off) {  // global_load ... v_off, s[base:base+1]
    return *reinterpret_cast<const T *>(static_cast<const char *>(base) + byte_off);
}

// outside the cube: every primitive (scene.ts:166,183-189), as all_prims_distance<0>.  Out of line and with plain
// arguments: a reference to the kernel's parameter block would force a copy of it into scratch.
__device__ __attribute__((noinline)) double oct_outside_distance(const RmSphere *spheres, const double *radii, int n, bool filter, float px,
                                                                 float py, float pz) {
    const Vec3f p = {px, py, pz};
    if (filter && n >= 2) return prims_min_best<int32_t>(spheres, radii, nullptr, n, 0, p, RM_MAX_DIST);
    return prims_min<true>(spheres, radii, static_cast<const int32_t *>(nullptr), n, p, RM_MAX_DIST, false);
}

// the near-tie pass of recs_min (another sphere may tie or win): ordinary filtered pass over the whole leaf, out of line
__device__ __attribute__((noinline)) double oct_leaf_rescan(const RmSphereRec *recs, int n, float px, float py, float pz, double closest) {
    const Vec3f p = {px, py, pz};
    float ub = f32_upper_bound(closest);
    for (int k = 0; k < n; ++k) rec_consider(*reinterpret_cast<const float4 *>(recs + k), recs + k, p, closest, ub);
    return closest;
}

__global__ __launch_bounds__(64, 8) void render_kernel_oct(const RmRenderParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tw = P.tile_w, th = 64 / tw;
    const int tiles_x = (P.width + tw - 1) / tw;
    const int tile = v1_tile_of_block(static_cast<int>(blockIdx.x));
    const int bx = tile % tiles_x, by = tile / tiles_x;
    const int x = bx * tw + (lane % tw);
    const int wpw = static_cast<int>(blockDim.x >> 6);             // waves per workgroup (the launcher uses 1)
    const int row = by * (wpw * th) + wave * th + (lane / tw);  // tile-local row
#ifdef RM_COUNTS
    if (threadIdx.x == 0) rm_cnt_g = P.stamps;
    __syncthreads();
#endif
    // (no early return: every wave takes part in the diagnostics flush at the end; a lane outside the frame starts finished)
    const bool in_frame = x < P.width && row < P.local_rows;
    if (in_frame) RM_CNT1(14)
    const int y = row_to_y(P, row);
    const Ray ray = make_ray(P, x, y);
    // 1 / direction (octree.ts:200) and, per axis, the byte offset inside RmOctNode of the face the ray leaves through
    // (lo: 0, hi: 16, + 4 per axis): `if (invDir < 0) swap(t0, t1)` (octree.ts:204-208) decided once per ray
    const double inv0 = 1.0 / static_cast<double>(ray.d.x), inv1 = 1.0 / static_cast<double>(ray.d.y), inv2 = 1.0 / static_cast<double>(ray.d.z);
    const uint32_t far0 = inv0 < 0.0 ? 0u : 32u, far1 = inv1 < 0.0 ? 8u : 40u, far2 = inv2 < 0.0 ? 16u : 48u;  // into RmOctFrameNode
    // tEnter needs no evaluation when tExit is clearly ahead.  The march point p = fl32(o + d t) lies inside the leaf's box
    // (findNode), so on every axis the ray's real entry parameter is at most t + eps / |d_a| with eps < 6e-7 (the binary32
    // rounding of a coordinate of magnitude <= 10; the binary64 roundings are nine orders smaller), and the computed tMin of
    // that axis exceeds the real one by < 1e-7 relative (two binary64 roundings, one binary32).  With
    // E = 4e-6 max_a |1 / d_a| (>= 4e-6): tEnter <= (t + 0.15 E)(1 + 1e-7) < t + E for t <= 10 (0.85 E > 1.01e-6), so `tEnter > tExit`
    // (octree.ts:215) is false when tExit - t > E.  A zero direction component makes E infinite: such rays always take the full test.
    const double near_margin = 4e-6 * __builtin_fmax(__builtin_fmax(__builtin_fabs(inv0), __builtin_fabs(inv1)), __builtin_fabs(inv2));

    enum { PH_MARCH = 0, PH_N0 = 1, PH_N1 = 2, PH_N2 = 3, PH_N3 = 4, PH_DONE = 5 };
    // Registers decide the occupancy here (64 VGPRs: eight waves per SIMD).  The two Uint16Array counters share one: the march
    // iterations (<= 100) in the low half, the SDF evaluations in the high half, where `+=` wraps exactly as the Uint16Array
    // store would (raymarcher.ts:103-106).  The trip counter of the march loop rides above the phase (phase in bits 0-2).
    uint32_t counters = 0;
    int phase = in_frame ? PH_MARCH : PH_DONE;  // | steps << 3
    double t = 0.0, d0 = 0.0;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    const void *const nodes = P.oct;
    const void *const frame = P.oct_frame;
    // One structured body per trip (no `continue` / `break`: each of them costs a loop level of mask bookkeeping in the
    // compiled code): a trip either skips, or evaluates one distance and consumes it according to the ray's phase.
    while (phase != PH_DONE) {
        RM_CNT1(0)
        asm volatile("" : "+v"(phase));  // opaque across the back edge: otherwise the optimiser threads the known phase values through
                                         // the loop and the structuriser turns the result into a six-deep loop nest
        if ((phase & 7) == PH_MARCH) {
            if (phase >= (RM_MAX_STEPS << 3)) phase = (t >= RM_MAX_DIST) ? PH_DONE : PH_N0;  // loop exhausted: return totalDist
            else phase += 8;
        }
        if (phase != PH_DONE) {
            // the march point (sphereTracer.ts:44-45), the hit position (raymarcher.ts:94-95) or one of getNormal's offsets (:126-131)
            Vec3f p = point_at(ray, t);
            if (static_cast<unsigned>(phase) - PH_N1 <= static_cast<unsigned>(PH_N3 - PH_N1)) {  // x - 0.01 in binary64, stored to the Float32Array; x - 0.0 is x
                p.x = to_f32(static_cast<double>(p.x) - (phase == PH_N1 ? 0.01 : 0.0));
                p.y = to_f32(static_cast<double>(p.y) - (phase == PH_N2 ? 0.01 : 0.0));
                p.z = to_f32(static_cast<double>(p.z) - (phase == PH_N3 ? 0.01 : 0.0));
            }
            double dist = RM_MAX_DIST;
            bool evaluated = true;
            const float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(p.x), __builtin_fabsf(p.y)), __builtin_fabsf(p.z));
            if (m <= 10.0f) {  // Octree.findNode through the cell table
                const uint32_t cell = (oct_cell_up(p.z) * 64u + oct_cell_up(p.y)) * 64u + oct_cell_up(p.x);
                const uint32_t node = static_cast<uint32_t>(ld_off<int32_t>(P.oct_lut, cell * 4u));
                __builtin_assume(node < (1u << 24));
                const uint32_t nb = node * 64u;
                // one batch: the far faces and the skip cap of the frame's table, primCount / isEmpty, and what a leaf evaluation reads
                const double ff0 = ld_off<double>(frame, nb + far0), ff1 = ld_off<double>(frame, nb + far1), ff2 = ld_off<double>(frame, nb + far2);
                const double cap = ld_off<double>(frame, nb + 24u);  // minDistance * 0.99
                const int2 pc_ie = ld_off<int2>(nodes, nb + 40u);    // prim_count, is_empty
                const int prim_first = ld_off<int32_t>(nodes, nb + 28u);
                const float4 sub = ld_off<float4>(nodes, nb + 48u);  // sub-cells per unit length x 3, sub_first
                const int prim_count = pc_ie.x;
                if ((phase & 7) == PH_MARCH && pc_ie.y) {  // Octree.marchRay (octree.ts:250-294): skip the rest of an empty leaf
                    const float tf0 = to_f32(ff0 * inv0), tf1 = to_f32(ff1 * inv1), tf2 = to_f32(ff2 * inv2);  // (face - origin) * invDir
                    // JS: tExit = Math.min(...) is NaN when an operand is, and then no comparison holds: skip 0; a NaN tEnter is ignored
                    const bool tf_nan = (tf0 != tf0) | (tf1 != tf1) | (tf2 != tf2);
                    const float xt = __builtin_fminf(__builtin_fminf(tf0, tf1), tf2);
                    bool bad = tf_nan | (xt < 0.0f);
                    const double ahead = static_cast<double>(xt) - t;
                    if (!(ahead > near_margin)) {  // tExit is not clearly ahead (or NaN): the near faces decide (octree.ts:215)
                        const float tn0 = to_f32(ld_off<double>(frame, nb + (far0 ^ 32u)) * inv0), tn1 = to_f32(ld_off<double>(frame, nb + (far1 ^ 32u)) * inv1),
                                    tn2 = to_f32(ld_off<double>(frame, nb + (far2 ^ 32u)) * inv2);
                        const bool tn_nan = (tn0 != tn0) | (tn1 != tn1) | (tn2 != tn2);
                        const float et = __builtin_fmaxf(__builtin_fmaxf(tn0, tn1), tn2);
                        bad |= !tn_nan & (et > xt);
                    }
                    double step = __builtin_fmax(ahead, 0.0);  // Math.max(0, tExit - t)
                    step = step < cap ? step : cap;
                    if (!bad && step > 0.0) {
                        RM_CNT1(1)
                        t += step + 0.001;
                        if (t > RM_MAX_DIST) phase = PH_DONE;  // `break`: depth >= MAX_DIST, no normal
                        evaluated = false;                      // `continue`
                        // Skip chain: a skip that minDistance cut short leaves the ray INSIDE this empty leaf, and the next trips of
                        // the reference's loop find the same node and compute the same tExit -- only t differs.  While the
                        // new t is clearly short of tExit (by near_margin: the march point then lies inside the box by more than
                        // its binary32 rounding on every axis, so findNode returns this leaf again, and tEnter, which only shrinks
                        // relative to t, cannot exceed tExit), the next skip needs neither the cell table nor the node: it is
                        // min(tExit - t, cap) + 0.001 again.  Each is a trip of the march loop (sphereTracer.ts:43,59-64).
                        while (phase != PH_DONE && phase < (RM_MAX_STEPS << 3)) {
                            const double ahead2 = static_cast<double>(xt) - t;
                            if (!(ahead2 > near_margin)) break;
                            RM_CNT1(3)
                            phase += 8;
                            const double step2 = ahead2 < cap ? ahead2 : cap;  // ahead2 > 0; cap > 0 (step > 0 above)
                            t += step2 + 0.001;
                            if (t > RM_MAX_DIST) phase = PH_DONE;
                        }
                    }
                }
                if (evaluated) {
                    if (prim_count > 0) {
                        RM_CNT1(2)
                        counters += static_cast<uint32_t>(prim_count) << 16;
                        const uint32_t rb = static_cast<uint32_t>(prim_first) * 32u;  // the leaf's records (RmSphereRec, 32 B)
                        const float inf = __builtin_inff();
                        int k1 = 0;
                        float hi1 = inf, lb1 = inf, lb2 = inf;
                        auto scan = [&](const float4 c, int k) {  // as recs_min: the smallest upper bound, and the smallest lower bound of the others
                            const float dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
                            const float len = __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz);
                            const float err = (len + __builtin_fabsf(c.w) + 1.0f) * 4e-6f;  // sphere_sdf_estimate
                            const float a = len - c.w, lb = a - err, hi = a + err;
                            const bool better = hi < hi1;
                            const float other = better ? lb1 : lb;  // (no NaN here: finite point, finite spheres)
                            lb2 = other < lb2 ? other : lb2;
                            k1 = better ? k : k1;
                            lb1 = better ? lb : lb1;
                            hi1 = better ? hi : hi1;
                        };
                        const int sub_first = __builtin_bit_cast(int32_t, sub.w);
                        if (P.oct_sub_hdr && sub_first >= 0) {  // crowded leaf: the candidates of p's sub-cell
                            const float lo0 = ld_off<float>(nodes, nb), lo1 = ld_off<float>(nodes, nb + 4u), lo2 = ld_off<float>(nodes, nb + 8u);
                            const int sx = min(max(static_cast<int>((p.x - lo0) * sub.x), 0), RM_OCT_SUB - 1);
                            const int sy = min(max(static_cast<int>((p.y - lo1) * sub.y), 0), RM_OCT_SUB - 1);
                            const int sz = min(max(static_cast<int>((p.z - lo2) * sub.z), 0), RM_OCT_SUB - 1);
                            const uint32_t sc = __umul24(__umul24(static_cast<uint32_t>(sz), RM_OCT_SUB) + static_cast<uint32_t>(sy), RM_OCT_SUB) +
                                                static_cast<uint32_t>(sx);  // 24-bit multiplies: full rate, v_mul_lo_u32 is not
                            const uint32_t hdr = ld_off<uint32_t>(P.oct_sub_hdr, (static_cast<uint32_t>(sub_first) + sc) * 4u);
                            const uint32_t lb0 = hdr >> 8;
                            const int n_sub = static_cast<int>(hdr & 0xFFu);
                            for (int e = 0; e < n_sub; ++e) {
                                RM_CNT1(6)
                                const int j = ld_off<uint8_t>(P.oct_sub_list, lb0 + static_cast<uint32_t>(e));
                                scan(ld_off<float4>(P.oct_recs, rb + static_cast<uint32_t>(j) * 32u), j);
                            }
                        } else {
                            for (int k = 0; k < prim_count; ++k) {
                                RM_CNT1(7)
                                scan(ld_off<float4>(P.oct_recs, rb + static_cast<uint32_t>(k) * 32u), k);
                            }
                        }
                        RM_CNT1(8)
                        const float4 c = ld_off<float4>(P.oct_recs, rb + static_cast<uint32_t>(k1) * 32u);
                        const double e =
                            vec3_length(p.x - c.x, p.y - c.y, p.z - c.z) - ld_off<double>(P.oct_recs, rb + static_cast<uint32_t>(k1) * 32u + 16u);
                        dist = e < dist ? e : dist;
                        if (lb2 <= f32_upper_bound(dist)) {
                            RM_CNT1(9)
                            dist = oct_leaf_rescan(P.oct_recs + prim_first, prim_count, p.x, p.y, p.z, dist);
                        }
                    } else if (pc_ie.y) {
                        RM_CNT1(11)
                        dist = min_dist(cap, dist);  // Math.min(closest, minDistance * safety) (scene.ts:160-163)
                    }
                }
            } else {
                RM_CNT1(12)
                counters += static_cast<uint32_t>(P.n_prims) << 16;
                dist = oct_outside_distance(P.spheres, P.radii, P.n_prims, P.filter != 0, p.x, p.y, p.z);
            }
            if (evaluated) {
                if ((phase & 7) == PH_MARCH) {
                    t += dist;
                    counters += 1;
                    if (dist < RM_EPSILON || t > RM_MAX_DIST) phase = (t >= RM_MAX_DIST) ? PH_DONE : PH_N0;  // raymarcher.ts:97-99
                } else if (phase == PH_N0) {
                    RM_CNT1(13)
                    d0 = dist;
                    phase = PH_N1;
                } else if (phase == PH_N1) {
                    nx = to_f32(d0 - dist);
                    phase = PH_N2;
                } else if (phase == PH_N2) {
                    ny = to_f32(d0 - dist);
                    phase = PH_N3;
                } else {
                    nz = to_f32(d0 - dist);
                    normalize3(nx, ny, nz);
                    phase = PH_DONE;
                }
            }
        }
    }
    if (in_frame) store_pixel(P, static_cast<size_t>(row) * P.width + x, t, nx, ny, nz, counters >> 16, counters & 0xFFFFu);
    v1_diag_epilogue(P.diag_block, P.diag_out, in_frame, counters >> 16, counters & 0xFFFFu);
}

#endif  // !RM_RTC

// diag: where the diagnostics of this workgroup's pixels are accumulated (null: nowhere), result to P.diag_out
template <int ACCEL, bool OTHER, int GEN, typename BLK>
__device__ __forceinline__ void render_body(const RmRenderParams &P, BLK *diag) {
    // wave tile: tile_w x (64 / tile_w); the waves of a workgroup (blockDim / 64: option `v1_block`) stacked vertically
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tw = P.tile_w, th = 64 / tw;
    const int tiles_x = (P.width + tw - 1) / tw;
    const int tile = v1_tile_of_block(static_cast<int>(blockIdx.x));
    const int bx = tile % tiles_x, by = tile / tiles_x;
    const int x = bx * tw + (lane % tw);
    const int row = by * (static_cast<int>(blockDim.x >> 6) * th) + wave * th + (lane / tw);  // tile-local row
    const int rows = P.local_rows;
#ifdef RM_COUNTS
    if (threadIdx.x == 0) rm_cnt_g = P.stamps;
    __syncthreads();
#endif
    const bool in_frame = x < P.width && row < rows;  // (no early return: the diagnostics flush at the end takes every wave)
    uint16_t c16 = 0, i16 = 0;
    if (in_frame) {
    RM_CNT1(14)
    const int y = row_to_y(P, row);
    const size_t idx = static_cast<size_t>(row) * P.width + x;

    // raymarcher.ts:73,83-88
    const double v = (static_cast<double>(y) / static_cast<double>(P.height) - 0.5) * 2.0;
    const double u = (static_cast<double>(x) / static_cast<double>(P.width) - 0.5) * 2.0;
    const double ax = to_f32(u), ay = to_f32(v), az = -1.0;
    float dx = to_f32(ax * P.rot[0] + ay * P.rot[3] + az * P.rot[6]);
    float dy = to_f32(ax * P.rot[1] + ay * P.rot[4] + az * P.rot[7]);
    float dz = to_f32(ax * P.rot[2] + ay * P.rot[5] + az * P.rot[8]);
    double len = static_cast<double>(dx) * dx + static_cast<double>(dy) * dy + static_cast<double>(dz) * dz;
    if (len > 0) len = 1 / __builtin_sqrt(len);
    Ray ray;
    ray.d.x = to_f32(dx * len);
    ray.d.y = to_f32(dy * len);
    ray.d.z = to_f32(dz * len);
    ray.o.x = P.origin[0];
    ray.o.y = P.origin[1];
    ray.o.z = P.origin[2];
    ray.od[0] = P.origin_d[0];
    ray.od[1] = P.origin_d[1];
    ray.od[2] = P.origin_d[2];

    uint32_t count = 0, iters = 0;
    const double depth = OTHER ? ray_march_other<ACCEL, GEN>(P, ray, count, iters) : ray_march<ACCEL, GEN>(P, ray, count, iters);
    uint8_t nb[3];
    normal_and_store<ACCEL, GEN>(P, ray, depth, count, nb);
    const uint8_t db = u8clamp(depth);
    c16 = static_cast<uint16_t>(count & 0xFFFFu);  // Uint16Array += wraps
    i16 = static_cast<uint16_t>(iters & 0xFFFFu);
    if (P.depth) P.depth[idx] = db;
    if (P.normal) {
        P.normal[3 * idx] = nb[0];
        P.normal[3 * idx + 1] = nb[1];
        P.normal[3 * idx + 2] = nb[2];
    }
    if (P.sdf) P.sdf[idx] = c16;
    if (P.iters) P.iters[idx] = i16;
    if (P.rgba) reinterpret_cast<uchar4 *>(P.rgba)[idx] = shade_pixel(P.shader, db, nb[0], nb[1], nb[2], c16, i16, P.light_d);
    }
    v1_diag_epilogue(diag, P.diag_out, in_frame, c16, i16);
}

template <int ACCEL, int GEN>
__device__ __forceinline__ void distance_body(const RmRenderParams &P, const float *pts, int64_t n, double *dist, uint32_t *count) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Vec3f p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    uint32_t c = 0;
    dist[i] = scene_distance<ACCEL, GEN>(P, p, c);
    count[i] = c;
}

#ifdef RM_RTC
}  // namespace
extern "C" __global__ __launch_bounds__(256) void rm_rtc_render(const RmRenderParams P) { render_body<RM_RTC_ACCEL, RM_RTC_OTHER != 0, 4>(P, P.diag_block); }
extern "C" __global__ __launch_bounds__(256) void rm_rtc_distance(const RmRenderParams P, const float *pts, int64_t n, double *dist, uint32_t *count) {
    distance_body<RM_RTC_ACCEL, 4>(P, pts, n, dist, count);
}
#else
template <int ACCEL, bool OTHER, int GEN>
__global__ __launch_bounds__(256) void render_kernel(const RmRenderParams P) {
    render_body<ACCEL, OTHER, GEN>(P, P.diag_block);
}

// ------------------------------------------------------------------ many frames of one scene in one launch
//
// rm_render_frames_device: blockIdx.y numbers the frame, blockIdx.x the frame's tiles exactly as render_kernel's does.  What a
// frame has of its own -- camera, time, where its pixels and its diagnostics go -- is taken from views[blockIdx.y] and written
// over a copy of the parameter block; everything else is the launch's.  blockIdx.y is the same for every lane, the table is
// read before the kernel stores anything and each word passes through readfirstlane, so the frame's state lives in scalar
// registers like the parameter block it replaces (no per-lane camera loads; the copy itself dissolves into registers).
__device__ __forceinline__ float frame_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ double frame_uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned int lo = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(b)));
    const unsigned int hi = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(b >> 32)));
    return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
}

template <int ACCEL, bool OTHER, int GEN>
__global__ __launch_bounds__(256) void frames_kernel(const RmRenderParams P, const RmFrameView *__restrict__ views, RmFrameDiagBlock *blocks,
                                                     RmDiagDevice *acc) {
    const unsigned int f = blockIdx.y;
    const RmFrameView *V = views + f;
    RmRenderParams Q = P;
#pragma unroll
    for (int k = 0; k < 9; ++k) Q.rot[k] = frame_uniform(V->rot[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Q.origin[k] = frame_uniform(V->origin[k]);
        Q.origin_d[k] = frame_uniform(V->origin_d[k]);
    }
    Q.time = frame_uniform(V->time);
    const size_t first = static_cast<size_t>(f) * (static_cast<size_t>(P.width) * static_cast<size_t>(P.local_rows));  // the frame's first pixel
    if (P.depth) Q.depth = P.depth + first;
    if (P.normal) Q.normal = P.normal + 3 * first;
    if (P.sdf) Q.sdf = P.sdf + first;
    if (P.iters) Q.iters = P.iters + first;
    if (P.rgba) Q.rgba = P.rgba + 4 * first;
    Q.diag_out = acc ? acc + f : nullptr;
    render_body<ACCEL, OTHER, GEN>(Q, blocks ? blocks + f : nullptr);
}

#ifndef RM_LENGTH_SQRT  // scene-independent kernels exist once (this file is compiled a second time with -DRM_LENGTH_SQRT)
// ------------------------------------------------------------------ small kernels

// The octree's boxes relative to one camera position (render_kernel_oct): intersectRayBox computes (bounds - origin) * invDir
// per ray and axis (octree.ts:200-203); the difference does not depend on the ray.
__global__ __launch_bounds__(256) void oct_frame_table_kernel(const RmOctNode *nodes, int n, double ox, double oy, double oz,
                                                              RmOctFrameNode *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RmOctNode nd = nodes[i];
    RmOctFrameNode f;
    f.lo[0] = static_cast<double>(nd.lo[0]) - ox;
    f.lo[1] = static_cast<double>(nd.lo[1]) - oy;
    f.lo[2] = static_cast<double>(nd.lo[2]) - oz;
    f.cap = nd.min_distance * 0.99;
    f.hi[0] = static_cast<double>(nd.hi[0]) - ox;
    f.hi[1] = static_cast<double>(nd.hi[1]) - oy;
    f.hi[2] = static_cast<double>(nd.hi[2]) - oz;
    f.pad = 0.0;
    out[i] = f;
}

__global__ __launch_bounds__(256) void shade_kernel(int shader, int64_t n, const uint8_t *depth, const uint8_t *normal,
                                                    const uint16_t *sdf, const uint16_t *iters, uchar4 *rgba, float l0,
                                                    float l1, float l2) {
    const double light[3] = {l0, l1, l2};
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        rgba[i] = shade_pixel(shader, depth[i], normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], sdf[i], iters[i],
                              light);
    }
}

__global__ __launch_bounds__(256) void reduce_kernel(const uint16_t *sdf, const uint16_t *iters, int64_t n,
                                                     RmDiagDevice *acc) {
    unsigned long long s = 0, it = 0;
    unsigned int mx = 0, mn = 0xFFFFFFFFu;
    const int64_t tid = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int64_t nthreads = static_cast<int64_t>(gridDim.x) * blockDim.x;
    int64_t done = 0;
    // 16-byte loads (8 counters per lane per load) when both streams are 16-byte aligned
    if (((reinterpret_cast<uintptr_t>(sdf) | reinterpret_cast<uintptr_t>(iters)) & 15) == 0) {
        const int64_t nvec = n / 8;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(sdf);
        const uint4 *i4 = reinterpret_cast<const uint4 *>(iters);
        auto eat = [&](const uint4 a, const uint4 b) {
            const unsigned int aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned int lo = aw[k] & 0xFFFFu, hi = aw[k] >> 16;
                s += lo + hi;
                mx = lo > mx ? lo : mx;
                mx = hi > mx ? hi : mx;
                mn = lo < mn ? lo : mn;
                mn = hi < mn ? hi : mn;
                it += (bw[k] & 0xFFFFu) + (bw[k] >> 16);
            }
        };
        int64_t v = tid;
        for (; v + 3 * nthreads < nvec; v += 4 * nthreads) {  // eight 16-B loads in flight per lane
            const uint4 a0 = s4[v], b0 = i4[v], a1 = s4[v + nthreads], b1 = i4[v + nthreads];
            const uint4 a2 = s4[v + 2 * nthreads], b2 = i4[v + 2 * nthreads], a3 = s4[v + 3 * nthreads], b3 = i4[v + 3 * nthreads];
            eat(a0, b0);
            eat(a1, b1);
            eat(a2, b2);
            eat(a3, b3);
        }
        for (; v < nvec; v += nthreads) eat(s4[v], i4[v]);
        done = nvec * 8;
    }
    for (int64_t i = done + tid; i < n; i += nthreads) {
        const unsigned int c = sdf[i];
        s += c;
        it += iters[i];
        mx = c > mx ? c : mx;
        mn = c < mn ? c : mn;
    }
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        it += __shfl_down(it, off);
        const unsigned int omx = __shfl_down(mx, off), omn = __shfl_down(mn, off);
        mx = omx > mx ? omx : mx;
        mn = omn < mn ? omn : mn;
    }
    // one atomic set per workgroup: the four words share a cache line, so per-wave atomics from
    // thousands of waves serialise (measured: 0.39 ms for 8192 waves vs the ~15 us the loads take)
    __shared__ unsigned long long sh_s[4], sh_it[4];
    __shared__ unsigned int sh_mx[4], sh_mn[4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_s[w] = s;
        sh_it[w] = it;
        sh_mx[w] = mx;
        sh_mn[w] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            s += sh_s[k];
            it += sh_it[k];
            mx = sh_mx[k] > mx ? sh_mx[k] : mx;
            mn = sh_mn[k] < mn ? sh_mn[k] : mn;
        }
        atomicAdd(&acc->total_sdf, s);
        atomicAdd(&acc->total_iters, it);
        atomicMax(&acc->max_sdf, mx);
        atomicMin(&acc->min_sdf, mn);
    }
}

__global__ void reduce_init_kernel(RmDiagDevice *acc) {
    acc->total_sdf = 0;
    acc->total_iters = 0;
    acc->max_sdf = 0;
    acc->min_sdf = 0xFFFFFFFFu;
    acc->pad = 0;
}

// rm_render_frames_device for frames without a pixel: the neutral elements for all n accumulators (there is no render launch)
__global__ __launch_bounds__(256) void frames_neutral_kernel(RmDiagDevice *acc, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    acc[i].total_sdf = 0;
    acc[i].total_iters = 0;
    acc[i].max_sdf = 0;
    acc[i].min_sdf = 0xFFFFFFFFu;
    acc[i].pad = 0;
}
#endif  // !RM_LENGTH_SQRT

template <int ACCEL, int GEN>
__global__ __launch_bounds__(256) void distance_kernel(const RmRenderParams P, const float *pts, int64_t n, double *dist,
                                                       uint32_t *count) {
    distance_body<ACCEL, GEN>(P, pts, n, dist, count);
}

// ------------------------------------------------------------------ field queries (rm_scene_field)
//
// Scene.getDistance at the points of a lattice the lanes form themselves (include/rm_raymarch.h has the rule): lane r of the
// range takes the point of linear index A.first + r -- 64 consecutive i per wave --, forms each component in binary64 left to
// right with one rounding to binary32 (no contraction: -ffp-contract=off) and calls the scene_distance every other kernel
// calls.  Outputs are indexed by r, each may be null.  (8 x 8 tiles of (i, j) per wave were measured and lost: DESIGN.md 4.)
// The bodies of the field, tile and point kernels are device functions: the kernels of a scene's own field (field_kernel<ACCEL,
// GEN>, ...) and those of the exact field (field_exact_kernel<GEN>, ...: ACCEL = RM_ACCEL_EXACT, sphere and primitive records
// only -- expression programs have no tree to walk and run the acceleration-None instantiation, which evaluates every object)
// instantiate them.

// The lattice's point with index (fi, fj, fk): the rule's three components (rm_kernels.h, rm_lattice_component), each rounded
// once to binary32.  What the field, block, tile and sharp-vertex kernels evaluate the scene at.
__device__ __forceinline__ Vec3f lattice_point(const RmLattice &l, double fi, double fj, double fk) {
    return Vec3f{static_cast<float>(rm_lattice_component(l, 0, fi, fj, fk)), static_cast<float>(rm_lattice_component(l, 1, fi, fj, fk)),
                 static_cast<float>(rm_lattice_component(l, 2, fi, fj, fk))};
}

template <int ACCEL, int GEN>
__device__ __forceinline__ void field_body(const RmRenderParams &P, const RmFieldArgs &A) {
    const unsigned long long r = ((static_cast<unsigned long long>(A.block_first) + blockIdx.x) << 8) + threadIdx.x;
    if (r >= static_cast<unsigned long long>(A.n)) return;
    const unsigned long long l = static_cast<unsigned long long>(A.first) + r, row = l / A.nu, k = row / A.nv;
    const double fi = static_cast<double>(l - row * A.nu), fj = static_cast<double>(row - k * A.nv), fk = static_cast<double>(k);
    const Vec3f p = lattice_point(A.lat, fi, fj, fk);
    uint32_t c = 0;
    const double d = scene_distance<ACCEL, GEN>(P, p, c);
    if (A.dist) A.dist[r] = d;
    if (A.dist32) A.dist32[r] = static_cast<float>(d);
    if (A.count) A.count[r] = c;
}
template <int ACCEL, int GEN>
__global__ __launch_bounds__(256) void field_kernel(const RmRenderParams P, const RmFieldArgs A) {
    field_body<ACCEL, GEN>(P, A);
}
template <int GEN>
__global__ __launch_bounds__(256) void field_exact_kernel(const RmRenderParams P, const RmFieldArgs A) {
    field_body<3, GEN>(P, A);
}

// ------------------------------------------------------------------ object picking (rm_ray_pick)

// Primitive.sdf of device object `id`, bit-identical to the value the render's Scene.getDistance paths take for it (the
// filtered loops and the leaf records evaluate the same expressions: sphere_sdf_fast, prim_sdf_general, program_sdf).
template <int GEN>
__device__ __forceinline__ double pick_sdf(const RmRenderParams &P, int id, const Vec3f &p) {
    if (GEN >= 2) {  // one object at a time through the scalar cache: list_min's waterfall over the lanes' distinct ids
        double d = 0.0;
        for (bool done = false; !done;) {
            const int u = __builtin_amdgcn_readfirstlane(id);
            if (id == u) {
                d = program_sdf<GEN == 3>(P.prog, P.obj_ranges[2 * u], P.obj_ranges[2 * u + 1], p, P.time, P.prog_slots);
                done = true;
            }
        }
        return d;
    }
    if (GEN == 1) return prim_sdf_general(P.prims[id], p);
    return sphere_sdf_fast(P.spheres[id], P.radii[id], p);
}

// The candidates ids[0 .. n) (0 .. n-1 when ids is null) against the running minimum `best` and its object `obj`: the
// minimum is Scene.getDistance's (start 10; Math.min, which propagates NaN for expression programs, v_min_f64 -- NaN
// ignored -- for the finite-input primitive records), and obj is the LOWEST object index whose value equals it under IEEE
// ==, or the lowest NaN one once the minimum is NaN.  Min is order independent, so the walk order does not matter.
// slot_obj (sphere scenes under the BVH: spheres are stored in leaf order) maps a device slot to its object index.
template <int GEN>
__device__ void pick_list(const RmRenderParams &P, const int32_t *ids, int n, const int32_t *slot_obj, const Vec3f &p, double &best,
                          int &obj) {
    for (int k = 0; k < n; ++k) {
        const int id = ids ? ids[k] : k;
        const double v = pick_sdf<GEN>(P, id, p);
        const int j = (GEN == 0 && slot_obj) ? slot_obj[id] : id;
        if (GEN >= 2 && v != v) {
            obj = (best != best && obj < j) ? obj : j;
            best = v;
        } else if (v < best) {
            best = v;
            obj = j;
        } else if (v == best) {
            obj = (obj >= 0 && obj < j) ? obj : j;
        }
    }
}

// Whether no primitive inside the box lo .. hi can be nearer to (x, y, z) than `best`: the box is farther, by a margin of 2^-20,
// relative and absolute, for the binary32 boxes and the roundings of the distance itself.  Strict: a primitive that ties
// `best` is never pruned.  A point outside a primitive's padded box is outside the primitive, at least the box's distance
// away; a point INSIDE the box may be inside the primitive, as deep as the primitive is large, and there the box says nothing
// against a negative `best` (two overlapping spheres: once the first gave a negative value, the inequality alone prunes the
// box of the second, whose distance is 0, though the point may lie deeper in it).  OUTSIDE_ONLY prunes only boxes that do not
// contain the point.  The coarse pass of the sparse mesher keeps the inequality alone, as it was written.
template <bool OUTSIDE_ONLY>
__device__ __forceinline__ bool box_beyond(const float lo[3], const float hi[3], double x, double y, double z, double best) {
    const double ex = __builtin_fmax(__builtin_fmax(static_cast<double>(lo[0]) - x, x - static_cast<double>(hi[0])), 0.0);
    const double ey = __builtin_fmax(__builtin_fmax(static_cast<double>(lo[1]) - y, y - static_cast<double>(hi[1])), 0.0);
    const double ez = __builtin_fmax(__builtin_fmax(static_cast<double>(lo[2]) - z, z - static_cast<double>(hi[2])), 0.0);
    const double db = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
    return (!OUTSIDE_ONLY || db > 0.0) && db * (1.0 - 0x1p-20) - 0x1p-20 > best;
}

// min(10, min over the objects ids[] names of Primitive.sdf(p)) by a pruned walk of the skip-linked boxes `nodes` around them
// (sphere and primitive records; the comment at bvh_exact_distance has the argument).  evaluated takes the evaluations made.
template <int GEN, bool OUTSIDE_ONLY>
__device__ double tree_exact_distance(const RmRenderParams &P, const RmBvhNode *nodes, int n_nodes, const int32_t *ids, const Vec3f &p,
                                      uint32_t &evaluated) {
    double best = RM_MAX_DIST;
    const double x = p.x, y = p.y, z = p.z;
    for (int i = 0; i < n_nodes;) {
        const RmBvhNode node = nodes[i];
        if (box_beyond<OUTSIDE_ONLY>(node.lo, node.hi, x, y, z, best)) {
            i = node.skip;
            continue;
        }
        if (node.leaf < 0) {
            i = i + 1;
            continue;
        }
        const int first = node.leaf >> 8, cnt = node.leaf & 0xFF;
        for (int k = 0; k < cnt; ++k) best = min_dist(pick_sdf<GEN>(P, ids[first + k], p), best);
        evaluated += static_cast<uint32_t>(cnt);
        i = node.skip;
    }
    return best;
}

// The object at a point (include/rm_raymarch.h, rm_ray_pick and rm_scene_points): the lowest-index candidate of
// Scene.getDistance at `hit` whose Primitive.sdf attains the distance; the walk forms that minimum again, so it takes no distance.
// The candidates are what getDistance evaluates there (scene.ts:144-190): the octree leaf's primitives (none for an empty
// leaf, all of them outside the cube), the primitives of every BVH leaf whose box contains the point (plain skip-linked
// walk; all of them when that set is empty), or all.  Not counted: the pick is no part of the reference's work.
template <int ACCEL, int GEN>
__device__ __forceinline__ int object_at(const RmRenderParams &P, const Vec3f &hit, const int32_t *slot_obj) {
    double best = RM_MAX_DIST;
    int obj = -1;
    if constexpr (ACCEL == 3) {  // option `exact`: every object is a candidate; the walk and the pruning of tree_exact_distance
        if (GEN < 2 && P.bvh_nodes > 0) {
            const double x = hit.x, y = hit.y, z = hit.z;
            for (int i = 0; i < P.bvh_nodes;) {
                const RmBvhNode node = P.bvh[i];
                if (box_beyond<true>(node.lo, node.hi, x, y, z, best)) {
                    i = node.skip;
                    continue;
                }
                if (node.leaf < 0) {
                    i = i + 1;
                    continue;
                }
                pick_list<GEN>(P, P.bvh_prims + (node.leaf >> 8), node.leaf & 0xFF, slot_obj, hit, best, obj);
                i = node.skip;
            }
            return obj;
        }
        pick_list<GEN>(P, nullptr, P.n_prims, slot_obj, hit, best, obj);
        return obj;
    }
    if (ACCEL == 1) {
        const int node = oct_find(P, hit);
        if (node < 0) pick_list<GEN>(P, nullptr, P.n_prims, slot_obj, hit, best, obj);
        else {
            const RmOctNode nd = P.oct[node];
            if (nd.prim_count > 0) pick_list<GEN>(P, P.oct_prims + nd.prim_first, nd.prim_count, slot_obj, hit, best, obj);
        }
        return obj;
    }
    if (ACCEL == 2) {
        int found = 0;
        for (int i = 0; i < P.bvh_nodes;) {
            const RmBvhNode node = P.bvh[i];
            if (!box_contains(node.lo, node.hi, hit)) {
                i = node.skip;
                continue;
            }
            if (node.leaf < 0) {
                i = i + 1;
                continue;
            }
            const int first = node.leaf >> 8, cnt = node.leaf & 0xFF;
            pick_list<GEN>(P, P.bvh_prims + first, cnt, slot_obj, hit, best, obj);
            found += cnt;
            i = node.skip;
        }
        if (found) return obj;
    }
    pick_list<GEN>(P, nullptr, P.n_prims, slot_obj, hit, best, obj);
    return obj;
}

// The object a ray hit: -1 for depth >= MAX_DIST, else the object at hitPosition = f32(o + d * depth) (hit_normal's point).
template <int ACCEL, int GEN>
__device__ __forceinline__ int hit_object(const RmRenderParams &P, const Ray &ray, double depth, const int32_t *slot_obj) {
    if (depth >= RM_MAX_DIST) return -1;
    Vec3f hit;
    hit.x = to_f32(static_cast<double>(ray.o.x) + static_cast<double>(ray.d.x) * depth);
    hit.y = to_f32(static_cast<double>(ray.o.y) + static_cast<double>(ray.d.y) * depth);
    hit.z = to_f32(static_cast<double>(ray.o.z) + static_cast<double>(ray.d.z) * depth);
    return object_at<ACCEL, GEN>(P, hit, slot_obj);
}

// ------------------------------------------------------------------ sparse meshes: the coarse pass and the tiles
//
// include/rm_raymarch.h ("sparse meshes") has the rule.  The coarse pass wants the EXACT field at a block's centre --
// min(10, min over all objects of Primitive.sdf), what an acceleration-None upload of the scene answers -- whatever structure the
// active scene has: a BVH or octree field is the marchers' bound and proves nothing about a block.  Under a BVH (sphere and
// primitive-record scenes) the minimum is found by a pruned walk of the skip-linked nodes: a primitive lies inside its leaf's
// box, so no primitive of a subtree is nearer than the subtree's box, and a subtree whose box is farther than the best value so
// far -- by a margin of 2^-20, relative and absolute, for the binary32 boxes and the roundings of the distance itself -- cannot
// lower it.  Math.min does not depend on the order, so the pruned minimum is the full one, bit for bit.
// (The walk itself is tree_exact_distance, with the point queries above: one text for this pass and for option `exact`.)
template <int GEN>
__device__ double bvh_exact_distance(const RmRenderParams &P, const Vec3f &p) {
    uint32_t evaluated = 0;
    return tree_exact_distance<GEN, false>(P, P.bvh, P.bvh_nodes, P.bvh_prims, p, evaluated);
}

// Option `exact` (include/rm_raymarch.h): E(x) = min(10, min over ALL objects of Primitive.sdf(x)) for the point, field and tile
// queries, whatever structure the scene has.  The launch names the tree to walk in P.bvh / P.bvh_prims / P.bvh_nodes -- the
// scene's own BVH or the exact tree the host built for an octree or None scene (rm_scene_host.h, ExactTree) -- and 0 nodes
// where there is none to walk (expression programs, non-rigid transforms, ...): every object then, as acceleration None.
// count takes the Primitive.sdf evaluations made.
template <int GEN>
__device__ double exact_distance(const RmRenderParams &P, const Vec3f &p, uint32_t &count) {
    if constexpr (GEN < 2) {
        if (P.bvh_nodes > 0) return tree_exact_distance<GEN, true>(P, P.bvh, P.bvh_nodes, P.bvh_prims, p, count);
    }
    return all_prims_distance<GEN>(P, p, count);
}

// One lane per block: the exact distance at the block's centre, the keep flag into slot (0 kept, -1 dropped; the scatter of
// rm_mesh_sparse.hip turns it into the rank) and the kept blocks of the workgroup into totals.
template <int GEN, bool WALK>
__global__ __launch_bounds__(256) void blocks_kernel(const RmRenderParams P, const RmBlocksArgs A) {
    __shared__ unsigned int s_kept[4];
    const unsigned int b = blockIdx.x * 256u + threadIdx.x;
    bool keep = false;
    if (b < A.n_blocks) {
        const unsigned int row = b / A.nbu, bx = b - row * A.nbu, bz = row / A.nbv, by = row - bz * A.nbv;
        const double fi = static_cast<double>(min(8u * bx + 4u, A.nu - 1u)), fj = static_cast<double>(min(8u * by + 4u, A.nv - 1u)),
                     fk = static_cast<double>(min(8u * bz + 4u, A.nw - 1u));
        const Vec3f p = lattice_point(A.lat, fi, fj, fk);
        uint32_t c = 0;
        const double d = WALK ? bvh_exact_distance<GEN>(P, p) : all_prims_distance<GEN>(P, p, c);
        keep = !(__builtin_fabs(d - A.iso) > A.bound);  // a NaN distance keeps the block
        if (A.dist) A.dist[b] = d;
        A.slot[b] = keep ? 0 : -1;
    }
    const unsigned long long kept = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) s_kept[threadIdx.x >> 6] = static_cast<unsigned int>(__popcll(kept));
    __syncthreads();
    if (threadIdx.x == 0) A.totals[blockIdx.x] = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
}

// One workgroup per kept block, three passes over the 729 points of its tile, a fastest: the scene_distance of field_kernel at
// the lattice's own points, so a tile holds what rm_scene_field returns there, bit for bit; a tile point beyond the lattice
// holds the quiet NaN 0x7FF8000000000000.  A wave's points lie in a box of 9 x 9 x 2 lattice steps: its BVH candidates are
// coherent.  Faces shared by two kept blocks are evaluated by both (729 evaluations for 512 points of a block's own).
//
// Option `exact` (ACCEL 3) with a tree to walk: the 729 points share a small box, so the workgroup culls the tree once.  Every
// lane forms E at the tile's centre point c (lattice point 8 b + 4 per axis, inside the lattice or not; the same walk in every
// lane, so the loads are broadcasts).  E is 1-Lipschitz where the tree is used -- a minimum of true distances and 10 -- so
// U = E(c) + A.radius bounds E on the whole tile (radius: 4 (|du| + |dv| + |dw|) and the roundings' slack, as the coarse pass's
// bound).  An object attains E at a tile point x only if its sdf(x) <= U, and sdf(x) is at least the distance from x to the
// object's leaf box, which is at least the gap between that box and the tile's box c +- A.half: leaves whose gap is positive and
// exceeds U, by the margins of box_beyond, are dropped, the objects of the others go to an LDS list, and each point takes list_min over it --
// Math.min does not depend on the order, so the value is E bit for bit.  Wave 0 culls 64 consecutive nodes a step: the nodes
// are in pre-order and a node's subtree ends at its skip link, so a dropped node rules out the nodes up to there (a prefix
// maximum over the lanes), and the next step starts behind whatever the step ruled out.  A list of more than
// RM_EXACT_LIST_CAP ids sends the workgroup's points through the per-lane walk.
#define RM_EXACT_LIST_CAP 1024
template <int ACCEL, int GEN>
__device__ __forceinline__ void tiles_body(const RmRenderParams &P, const RmTilesArgs &A) {
    const unsigned int r = blockIdx.x;
    const unsigned int b = static_cast<unsigned int>(A.list[r]);
    const unsigned int row = b / A.nbu, bx = b - row * A.nbu, bz = row / A.nbv, by = row - bz * A.nbv;
    double *out = A.tiles + static_cast<size_t>(r) * RM_SPARSE_TILE;
    bool from_list = false;
    int n_list = 0;
    const int32_t *cand = nullptr;
#ifndef RM_EXACT_NO_LIST  // (a measurement build: every point through the per-lane walk)
    if constexpr (ACCEL == 3 && GEN < 2) {
        __shared__ int32_t s_list[RM_EXACT_LIST_CAP];
        __shared__ int s_n, s_over;
        const double fi = static_cast<double>(8u * bx + 4u), fj = static_cast<double>(8u * by + 4u), fk = static_cast<double>(8u * bz + 4u);
        const Vec3f c = lattice_point(A.lat, fi, fj, fk);
        // (uniform; a centre beyond the lattice's last point may overflow binary32 where the lattice's own points do not: no list then)
        if (P.bvh_nodes > 0 && c.x - c.x == 0.f && c.y - c.y == 0.f && c.z - c.z == 0.f) {
            uint32_t unused = 0;
            const double U = tree_exact_distance<GEN, true>(P, P.bvh, P.bvh_nodes, P.bvh_prims, c, unused) + A.radius;
            if (threadIdx.x == 0) {
                s_n = 0;
                s_over = 0;
            }
            __syncthreads();
            if (threadIdx.x < 64u) {
                const int lane = static_cast<int>(threadIdx.x);
                const double lx = static_cast<double>(c.x) - A.half[0], hx = static_cast<double>(c.x) + A.half[0];
                const double ly = static_cast<double>(c.y) - A.half[1], hy = static_cast<double>(c.y) + A.half[1];
                const double lz = static_cast<double>(c.z) - A.half[2], hz = static_cast<double>(c.z) + A.half[2];
                for (int base = 0; base < P.bvh_nodes;) {
                    const int idx = base + lane;
                    int cover = 0, leaf = -1;  // cover: where the subtree of a dropped node ends
                    if (idx < P.bvh_nodes) {
                        const RmBvhNode node = P.bvh[idx];
                        const double ex = __builtin_fmax(__builtin_fmax(static_cast<double>(node.lo[0]) - hx, lx - static_cast<double>(node.hi[0])), 0.0);
                        const double ey = __builtin_fmax(__builtin_fmax(static_cast<double>(node.lo[1]) - hy, ly - static_cast<double>(node.hi[1])), 0.0);
                        const double ez = __builtin_fmax(__builtin_fmax(static_cast<double>(node.lo[2]) - hz, lz - static_cast<double>(node.hi[2])), 0.0);
                        const double gap = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
                        // (a box that touches the tile's box stays: U may be negative, and inside a box so may an sdf)
                        if (gap > 0.0 && gap * (1.0 - 0x1p-20) - 0x1p-20 > U) cover = node.skip;
                        else leaf = node.leaf;
                    }
                    int ruled = cover;  // inclusive prefix maximum of cover
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const int o = __shfl_up(ruled, d);
                        if (lane >= d) ruled = max(ruled, o);
                    }
                    const int before = __shfl_up(ruled, 1);
                    const bool live = lane == 0 || idx >= before;  // not inside a subtree an earlier lane's node dropped
                    if (live && leaf >= 0 && (leaf & 0xFF) > 0) {
                        const int first = leaf >> 8, cnt = leaf & 0xFF;
                        const int at = atomicAdd(&s_n, cnt);
                        if (at + cnt <= RM_EXACT_LIST_CAP)
                            for (int k = 0; k < cnt; ++k) s_list[at + k] = P.bvh_prims[first + k];
                        else s_over = 1;
                    }
                    base = max(base + 64, __shfl(ruled, 63));
                }
            }
            __syncthreads();
            from_list = s_over == 0;
            n_list = s_n;
            cand = s_list;
        }
    }
#endif
#pragma unroll 1
    for (unsigned int t = threadIdx.x; t < RM_SPARSE_TILE; t += 256u) {
        const unsigned int q = t / 9u, ta = t - q * 9u, tg = q / 9u, tb = q - tg * 9u;
        const unsigned int i = 8u * bx + ta, j = 8u * by + tb, k = 8u * bz + tg;
        double d = __longlong_as_double(0x7FF8000000000000ll);
        if (i < A.nu && j < A.nv && k < A.nw) {
            const double fi = static_cast<double>(i), fj = static_cast<double>(j), fk = static_cast<double>(k);
            const Vec3f p = lattice_point(A.lat, fi, fj, fk);
            uint32_t c = 0;
            if (from_list) d = list_min<GEN>(P, cand, n_list, p, RM_MAX_DIST);
            else d = scene_distance<ACCEL, GEN>(P, p, c);
        }
        out[t] = d;
    }
}
template <int ACCEL, int GEN>
__global__ __launch_bounds__(256) void tiles_kernel(const RmRenderParams P, const RmTilesArgs A) {
    tiles_body<ACCEL, GEN>(P, A);
}
template <int GEN>
__global__ __launch_bounds__(256) void tiles_exact_kernel(const RmRenderParams P, const RmTilesArgs A) {
    tiles_body<3, GEN>(P, A);
}

// rm_scene_tiles_update_device (include/rm_raymarch.h, "re-meshing an edited scene"; DESIGN.md 4 has the argument): the exact
// tiles of the ACTIVE scene from those of the previous one.  One workgroup per kept block, as tiles_exact_kernel, and one
// decision for the whole workgroup: the block's previous tile is COPIED unless a ball of the edit can reach it, and a reached
// block -- or one that had no tile -- is EVALUATED by tiles_body<3, GEN>, the code the full path runs.  The previous tile is
// staged in LDS with coalesced loads (729 doubles; with tiles_body's candidate list the static LDS stays near 10 KB); M, the
// largest previous value at the tile's points inside the lattice, and the NaN flag are reduced across the four waves; the balls
// are dealt to the lanes, strided over 256, and a workgroup-wide OR says whether one reaches.  Every changed object version o
// has sdf_o(x) >= gap(ball, tile box) - rho at every tile point x, so with gap - rho > M (by the margins of box_beyond) none
// attains the old minimum and none can lower it: the new value is the old one, bit for bit.  A NaN anywhere evaluates.
template <int GEN>
__global__ __launch_bounds__(256) void tiles_update_kernel(const RmRenderParams P, const RmTilesArgs A, const RmTilesUpdateArgs U) {
    __shared__ double s_tile[RM_SPARSE_TILE];
    __shared__ double s_max[4];
    __shared__ int s_flag[4];
    const unsigned int r = blockIdx.x;
    const unsigned int b = static_cast<unsigned int>(A.list[r]);
    // (uniform from here to the branch: b, p and c are the same in every lane)
    const int p = b < U.n_blocks ? U.prev_slot[b] : -1;
    bool evaluate = p < 0 || static_cast<unsigned int>(p) >= U.n_prev_kept;
    const unsigned int row = b / A.nbu, bx = b - row * A.nbu, bz = row / A.nbv, by = row - bz * A.nbv;
    const double fi = static_cast<double>(8u * bx + 4u), fj = static_cast<double>(8u * by + 4u), fk = static_cast<double>(8u * bz + 4u);
    const Vec3f c = lattice_point(A.lat, fi, fj, fk);  // tiles_body's centre point: not clamped to the lattice
    if (!(c.x - c.x == 0.f && c.y - c.y == 0.f && c.z - c.z == 0.f)) evaluate = true;
    if (!evaluate) {
        const double *src = U.prev_tiles + static_cast<size_t>(p) * RM_SPARSE_TILE;
        double m = -__builtin_inf();
        bool flag = false;  // first: a NaN at a point inside the lattice
#pragma unroll
        for (unsigned int t = threadIdx.x; t < RM_SPARSE_TILE; t += 256u) {
            const double v = src[t];
            s_tile[t] = v;
            const unsigned int q = t / 9u, ta = t - q * 9u, tg = q / 9u, tb = q - tg * 9u;
            if (8u * bx + ta < A.nu && 8u * by + tb < A.nv && 8u * bz + tg < A.nw) {
                flag = flag || v != v;
                m = __builtin_fmax(m, v);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = __builtin_fmax(m, __shfl_xor(m, d));
        const bool wave_flag = __ballot(flag) != 0ull;
        if ((threadIdx.x & 63u) == 0) {
            s_max[threadIdx.x >> 6] = m;
            s_flag[threadIdx.x >> 6] = wave_flag ? 1 : 0;
        }
        __syncthreads();
        const double M = __builtin_fmax(__builtin_fmax(s_max[0], s_max[1]), __builtin_fmax(s_max[2], s_max[3]));
        const bool any_nan = (s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3]) != 0;
        __syncthreads();  // s_flag is written again below
        const double lx = static_cast<double>(c.x) - A.half[0], hx = static_cast<double>(c.x) + A.half[0];
        const double ly = static_cast<double>(c.y) - A.half[1], hy = static_cast<double>(c.y) + A.half[1];
        const double lz = static_cast<double>(c.z) - A.half[2], hz = static_cast<double>(c.z) + A.half[2];
        flag = false;  // now: a ball reaches the tile
        for (int i = static_cast<int>(threadIdx.x); i < U.n_balls; i += 256) {
            const RmBall ball = U.balls[i];
            const double cx = static_cast<double>(ball.center[0]), cy = static_cast<double>(ball.center[1]), cz = static_cast<double>(ball.center[2]);
            const double ex = __builtin_fmax(__builtin_fmax(lx - cx, cx - hx), 0.0);
            const double ey = __builtin_fmax(__builtin_fmax(ly - cy, cy - hy), 0.0);
            const double ez = __builtin_fmax(__builtin_fmax(lz - cz, cz - hz), 0.0);
            const double gap = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
            flag = flag || !(gap * (1.0 - 0x1p-20) - 0x1p-20 - ball.radius > M);
        }
        const bool wave_reach = __ballot(flag) != 0ull;
        if ((threadIdx.x & 63u) == 0) s_flag[threadIdx.x >> 6] = wave_reach ? 1 : 0;
        __syncthreads();
        evaluate = any_nan || (s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3]) != 0;
    }
    if (threadIdx.x == 0 && U.reused) U.reused[r] = evaluate ? 0 : 1;
    if (evaluate) {
        tiles_body<3, GEN>(P, A);
    } else {
        double *out = A.tiles + static_cast<size_t>(r) * RM_SPARSE_TILE;
        for (unsigned int t = threadIdx.x; t < RM_SPARSE_TILE; t += 256u) out[t] = s_tile[t];
    }
}

// ------------------------------------------------------------------ point queries (rm_scene_points)
//
// Distance, gradient, object and projection onto the surface for caller-supplied points (include/rm_raymarch.h has the rule):
// one point per lane, in input order, the launch of every query without a ray (scene_launch).  A visit of a point is
// Scene.getDistance there and -- when a step or the normal is wanted -- getNormal's three further evaluations; the loop below
// is that visit, so the distance evaluation and the gradient have ONE call site each however many steps a lane takes (a copy
// of scene_distance per use would multiply the kernel as it would have light_body's marcher).  The last visit's gradient is the normal: a loop that ends on a
// zero gradient has it already.  Lanes that converge early idle until their wave's last lane has: neighbouring points of a
// mesh or a hit buffer take about the same number of steps, and compacting them would cost a pass through memory.  A lane
// reads its point before it writes anything, so A.position may be A.points.
template <int ACCEL, int GEN>
__device__ __forceinline__ void point_body(const RmRenderParams &P, const RmPointArgs &A) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    Vec3f p{A.points[3 * i], A.points[3 * i + 1], A.points[3 * i + 2]}, g{0.f, 0.f, 0.f};
    uint32_t count = 0;
    int32_t steps = 0;
    double d;
#pragma unroll 1
    for (;;) {
        d = scene_distance<ACCEL, GEN>(P, p, count);
        const double r = d - A.iso;
        const bool step = steps < A.snap_steps && __builtin_fabs(r) > A.snap_tol;  // (a NaN r: no step)
        if (!step && !A.want_normal) break;
        g = distance_gradient<ACCEL, GEN>(P, p, d, count);
        if (!step || (g.x == 0.f && g.y == 0.f && g.z == 0.f)) break;
        p.x = to_f32(static_cast<double>(p.x) + static_cast<double>(g.x) * -r);
        p.y = to_f32(static_cast<double>(p.y) + static_cast<double>(g.y) * -r);
        p.z = to_f32(static_cast<double>(p.z) + static_cast<double>(g.z) * -r);
        ++steps;
    }
    if (!A.want_normal) g = Vec3f{0.f, 0.f, 0.f};
    if (A.position) {
        A.position[3 * i] = p.x;
        A.position[3 * i + 1] = p.y;
        A.position[3 * i + 2] = p.z;
    }
    if (A.dist) A.dist[i] = d;
    if (A.normal) {
        A.normal[3 * i] = g.x;
        A.normal[3 * i + 1] = g.y;
        A.normal[3 * i + 2] = g.z;
    }
    if (A.steps) A.steps[i] = steps;
    if (A.count) A.count[i] = count;
    if (A.object) A.object[i] = object_at<ACCEL, GEN>(P, p, A.slot_obj);
}
template <int ACCEL, int GEN>
__global__ __launch_bounds__(256) void point_kernel(const RmRenderParams P, const RmPointArgs A) {
    point_body<ACCEL, GEN>(P, A);
}
template <int GEN>
__global__ __launch_bounds__(256) void point_exact_kernel(const RmRenderParams P, const RmPointArgs A) {
    point_body<3, GEN>(P, A);
}

// ------------------------------------------------------------------ sharp vertices (rm_scene_sharpen)
//
// Dual contouring's vertex for the cells of a mesh (include/rm_raymarch.h, "sharp meshes", has the rule; tests/sharp_model.py
// restates it): the point that minimises the distance to the tangent planes sampled at the cell's edge crossings.  A workgroup of
// 256 lanes takes RM_SHARP_CELLS = 64 consecutive vertices -- neighbouring cells, so the BVH walks of a wave stay coherent:
//   stage 1  the 512 corner evaluations, two per lane (a wave takes one corner of all 64 cells at a time), into LDS
//   stage 2  wave 0 compacts the crossing edges of the 64 cells in (cell, edge) order -- at most 768 --, then all lanes take them
//            in turn: the refinement's evaluations, the last one and the gradient's three, the point and the normal into LDS.  A
//            cell has 3 to 7 crossings: one lane per vertex would idle half the workgroup through the longest part.
//   stage 3  lanes 0 .. 63 accumulate their cell's records in edge order and solve: the order is fixed by the list, so the result
//            does not depend on which lane evaluated what.
// Counts are integers: the lanes add theirs to the cell's word in LDS.  scene_distance has one call site in the corner pass and
// one in the loop that refines a bracket and, on its last trip, evaluates the crossing itself; the gradient is point_body's
// distance_gradient (point_body says why the call sites are kept few).  binary64 throughout, no contraction.
struct SharpCell {
    unsigned int i, j, k;
    bool exists;
};
__device__ __forceinline__ SharpCell sharp_locate(const RmSharpArgs &A, long long l) {
    SharpCell c{0u, 0u, 0u, false};
    const unsigned long long n = static_cast<unsigned long long>(A.nu) * A.nv * A.nw;
    if (l < 0 || static_cast<unsigned long long>(l) >= n) return c;
    const unsigned long long key = static_cast<unsigned long long>(l), row = key / A.nu, k = row / A.nv;
    c.i = static_cast<unsigned int>(key - row * A.nu);
    c.j = static_cast<unsigned int>(row - k * A.nv);
    c.k = static_cast<unsigned int>(k);
    c.exists = c.i + 1u < A.nu && c.j + 1u < A.nv && c.k + 1u < A.nw;
    return c;
}
__device__ __forceinline__ bool sharp_finite(double x) { return x - x == 0.0; }
__device__ __forceinline__ bool sharp_finite(float x) { return x - x == 0.f; }
// one Jacobi rotation of the symmetric a and of the rows of V in the plane (p, q); r is the third index
template <int p, int q>
__device__ __forceinline__ void sharp_rotate(double (&a)[3][3], double (&V)[3][3]) {
    constexpr int r = 3 - p - q;
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    double t = 1.0 / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    if (!(theta >= 0.0)) t = -t;
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c, h = t * apq;
    a[p][p] = a[p][p] - h;
    a[q][q] = a[q][q] + h;
    a[p][q] = a[q][p] = 0.0;
    const double arp = c * a[r][p] - s * a[r][q], arq = s * a[r][p] + c * a[r][q];
    a[r][p] = a[p][r] = arp;
    a[r][q] = a[q][r] = arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = c * V[k][p] - s * V[k][q], vq = s * V[k][p] + c * V[k][q];
        V[k][p] = vp;
        V[k][q] = vq;
    }
}
// eigenpair y ahead of eigenpair x when its value is strictly greater
template <int x, int y>
__device__ __forceinline__ void sharp_order(double (&lam)[3], double (&V)[3][3]) {
    if (!(lam[y] > lam[x])) return;
    const double l = lam[x];
    lam[x] = lam[y];
    lam[y] = l;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = V[k][x];
        V[k][x] = V[k][y];
        V[k][y] = v;
    }
}

template <int ACCEL, int GEN>
__device__ __forceinline__ void sharp_body(const RmRenderParams &P, const RmSharpArgs &A) {
    __shared__ double s_val[8][RM_SHARP_CELLS];            // corner dx + 2 dy + 4 dz of every cell; NaN for a cell that does not exist
    __shared__ float s_rec[RM_SHARP_CROSSINGS][6];         // p and n of a crossing, in list order
    __shared__ unsigned short s_list[RM_SHARP_CROSSINGS];  // cell << 4 | edge; bit 15: dropped
    __shared__ unsigned int s_count[RM_SHARP_CELLS], s_first[RM_SHARP_CELLS], s_mask[RM_SHARP_CELLS], s_total;
    const unsigned int tid = threadIdx.x;
    const long long base = static_cast<long long>(blockIdx.x) * RM_SHARP_CELLS;
    if (tid < RM_SHARP_CELLS) s_count[tid] = 0u;
    __syncthreads();

    // stage 1: the corners
#pragma unroll 1
    for (unsigned int e = tid; e < 8u * RM_SHARP_CELLS; e += 256u) {
        const unsigned int cell = e & (RM_SHARP_CELLS - 1u), corner = e / RM_SHARP_CELLS;
        double d = __longlong_as_double(0x7FF8000000000000ll);
        if (base + cell < A.n) {
            const SharpCell c = sharp_locate(A, A.cells[base + cell]);
            if (c.exists) {
                const double fi = static_cast<double>(c.i + (corner & 1u)), fj = static_cast<double>(c.j + ((corner >> 1) & 1u)),
                             fk = static_cast<double>(c.k + (corner >> 2));
                const Vec3f p = lattice_point(A.lat, fi, fj, fk);
                uint32_t n = 0;
                d = scene_distance<ACCEL, GEN>(P, p, n);
                atomicAdd(&s_count[cell], n);
            }
        }
        s_val[corner][cell] = d;
    }
    __syncthreads();

    // stage 2: the crossing edges of the active cells, compacted in (cell, edge) order by wave 0
    if (tid < RM_SHARP_CELLS) {
        unsigned int inside = 0u, mask = 0u;
        bool finite = true;
#pragma unroll
        for (unsigned int n = 0; n < 8u; ++n) {
            const double v = s_val[n][tid];
            finite = finite && sharp_finite(v);
            inside |= (v < A.iso ? 1u : 0u) << n;
        }
        if (finite && inside != 0u && inside != 255u) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const int lo_axis = ax == 0 ? 1 : 0, hi_axis = ax == 2 ? 1 : 2;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int low = ((e & 1) << lo_axis) | ((e >> 1) << hi_axis), high = low | (1 << ax);
                    if (((inside >> low) ^ (inside >> high)) & 1u) mask |= 1u << (4 * ax + e);
                }
            }
        }
        const unsigned int mine = static_cast<unsigned int>(__popc(mask));
        unsigned int upto = mine;  // inclusive prefix sum over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int o = __shfl_up(upto, d);
            if (static_cast<int>(tid) >= d) upto += o;
        }
        unsigned int at = upto - mine;
        s_first[tid] = at;
        s_mask[tid] = mask;
        for (unsigned int b = 0; b < 12u; ++b)
            if ((mask >> b) & 1u) s_list[at++] = static_cast<unsigned short>((tid << 4) | b);
        if (tid == RM_SHARP_CELLS - 1u) s_total = upto;
    }
    __syncthreads();

    const unsigned int total = s_total;  // <= RM_SHARP_CROSSINGS: twelve bits per cell
#pragma unroll 1
    for (unsigned int x = tid; x < total; x += 256u) {
        const unsigned int entry = s_list[x], cell = entry >> 4, edge = entry & 15u, ax = edge >> 2, e = edge & 3u;
        const SharpCell c = sharp_locate(A, A.cells[base + cell]);
        const unsigned int lo_axis = ax == 0u ? 1u : 0u, hi_axis = ax == 2u ? 1u : 2u;
        const unsigned int low = ((e & 1u) << lo_axis) | ((e >> 1) << hi_axis), high = low | (1u << ax);
        const double a = s_val[low][cell], b = s_val[high][cell];
        const double bi = static_cast<double>(c.i + (low & 1u)), bj = static_cast<double>(c.j + ((low >> 1) & 1u)),
                     bk = static_cast<double>(c.k + (low >> 2));
        const bool a_inside = a < A.iso;
        double tl = 0.0, fl = a, th = 1.0, fh = b, d = 0.0;
        Vec3f p{0.f, 0.f, 0.f}, g{0.f, 0.f, 0.f};
        bool alive = true;
        uint32_t n = 0;
#pragma unroll 1
        for (int it = 0;; ++it) {  // R refinements of the bracket, then the crossing itself
            const double t = tl + (A.iso - fl) * (th - tl) / (fh - fl);
            const double fi = ax == 0u ? bi + t : bi, fj = ax == 1u ? bj + t : bj, fk = ax == 2u ? bk + t : bk;
            p = lattice_point(A.lat, fi, fj, fk);
            if (!(sharp_finite(t) && sharp_finite(p.x) && sharp_finite(p.y) && sharp_finite(p.z))) {
                alive = false;
                break;
            }
            const double f = scene_distance<ACCEL, GEN>(P, p, n);
            if (it >= A.refine) {
                d = f;
                break;
            }
            if ((f < A.iso) == a_inside) {
                tl = t;
                fl = f;
            } else {
                th = t;
                fh = f;
            }
        }
        if (alive) {
            g = distance_gradient<ACCEL, GEN>(P, p, d, n);
            alive = sharp_finite(g.x) && sharp_finite(g.y) && sharp_finite(g.z);
        }
        s_rec[x][0] = p.x;
        s_rec[x][1] = p.y;
        s_rec[x][2] = p.z;
        s_rec[x][3] = g.x;
        s_rec[x][4] = g.y;
        s_rec[x][5] = g.z;
        if (!alive) s_list[x] = static_cast<unsigned short>(entry | 0x8000u);
        atomicAdd(&s_count[cell], n);
    }
    __syncthreads();

    // stage 3: one lane per vertex
    if (tid >= RM_SHARP_CELLS || base + tid >= A.n) return;
    const long long v = base + tid;
    const SharpCell c = sharp_locate(A, A.cells[v]);
    double x[3] = {0.0, 0.0, 0.0};
    int32_t feature = -1;
    if (c.exists) {
        const double fi = static_cast<double>(c.i) + 0.5, fj = static_cast<double>(c.j) + 0.5, fk = static_cast<double>(c.k) + 0.5;
        // (the rule's components before their rounding: the solve is binary64 around the cell's centre)
        const double centre[3] = {rm_lattice_component(A.lat, 0, fi, fj, fk), rm_lattice_component(A.lat, 1, fi, fj, fk),
                                  rm_lattice_component(A.lat, 2, fi, fj, fk)};
        x[0] = centre[0];
        x[1] = centre[1];
        x[2] = centre[2];
        const unsigned int mask = s_mask[tid], first = s_first[tid], last = first + static_cast<unsigned int>(__popc(mask));
        double m[3] = {0.0, 0.0, 0.0};
        unsigned int kept = 0u;
        if (mask) {
            feature = 0;
            for (unsigned int q = first; q < last; ++q) {
                if (s_list[q] & 0x8000u) continue;
                m[0] = m[0] + static_cast<double>(s_rec[q][0]);
                m[1] = m[1] + static_cast<double>(s_rec[q][1]);
                m[2] = m[2] + static_cast<double>(s_rec[q][2]);
                ++kept;
            }
        }
        if (kept) {
            const double count = static_cast<double>(kept);
            m[0] = m[0] / count;
            m[1] = m[1] / count;
            m[2] = m[2] / count;
            double a[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
            double b[3] = {0.0, 0.0, 0.0};
            for (unsigned int q = first; q < last; ++q) {
                if (s_list[q] & 0x8000u) continue;
                const double px = s_rec[q][0], py = s_rec[q][1], pz = s_rec[q][2], nx = s_rec[q][3], ny = s_rec[q][4], nz = s_rec[q][5];
                a[0][0] = a[0][0] + nx * nx;
                a[0][1] = a[0][1] + nx * ny;
                a[0][2] = a[0][2] + nx * nz;
                a[1][1] = a[1][1] + ny * ny;
                a[1][2] = a[1][2] + ny * nz;
                a[2][2] = a[2][2] + nz * nz;
                const double s = (nx * (px - m[0]) + ny * (py - m[1])) + nz * (pz - m[2]);
                b[0] = b[0] + nx * s;
                b[1] = b[1] + ny * s;
                b[2] = b[2] + nz * s;
            }
            a[1][0] = a[0][1];
            a[2][0] = a[0][2];
            a[2][1] = a[1][2];
#pragma unroll 1
            for (int sweep = 0; sweep < 6; ++sweep) {
                sharp_rotate<0, 1>(a, V);
                sharp_rotate<0, 2>(a, V);
                sharp_rotate<1, 2>(a, V);
            }
            double lam[3] = {a[0][0], a[1][1], a[2][2]};
            sharp_order<0, 1>(lam, V);
            sharp_order<1, 2>(lam, V);
            sharp_order<0, 1>(lam, V);
            int r0 = 0;
            if (lam[0] > 0.0) {
                const double least = A.rank_tol * lam[0];
                r0 = (lam[0] > least ? 1 : 0) + (lam[1] > least ? 1 : 0) + (lam[2] > least ? 1 : 0);
            }
            double coef[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) coef[i] = ((V[0][i] * b[0] + V[1][i] * b[1]) + V[2][i] * b[2]) / lam[i];
            x[0] = m[0];
            x[1] = m[1];
            x[2] = m[2];
#pragma unroll
            for (int r = 3; r >= 1; --r) {
                if (feature != 0 || r0 < r) continue;
                double cand[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double acc = m[k];
#pragma unroll
                    for (int i = 0; i < r; ++i) acc = acc + V[k][i] * coef[i];
                    cand[k] = acc;
                }
                const double dx = cand[0] - centre[0], dy = cand[1] - centre[1], dz = cand[2] - centre[2];
                if (__builtin_sqrt((dx * dx + dy * dy) + dz * dz) <= A.limit) {
                    x[0] = cand[0];
                    x[1] = cand[1];
                    x[2] = cand[2];
                    feature = r;
                }
            }
        }
    }
    A.position[3 * v] = static_cast<float>(x[0]);
    A.position[3 * v + 1] = static_cast<float>(x[1]);
    A.position[3 * v + 2] = static_cast<float>(x[2]);
    if (A.feature) A.feature[v] = feature;
    if (A.count) A.count[v] = s_count[tid];
}
template <int ACCEL, int GEN>
__global__ __launch_bounds__(256) void sharp_kernel(const RmRenderParams P, const RmSharpArgs A) {
    sharp_body<ACCEL, GEN>(P, A);
}
template <int GEN>
__global__ __launch_bounds__(256) void sharp_kernel_exact(const RmRenderParams P, const RmSharpArgs A) {
    sharp_body<3, GEN>(P, A);
}

// ------------------------------------------------------------------ ray queries (rm_ray_march, rm_ray_pick)

// Raymarcher.rayMarch (+ getNormal) for caller-supplied rays: one ray per lane, in input order.  The march is render_body's
// (ray_march / ray_march_other, same scene fields, the per-ray BVH hit-leaf list in dynamic LDS); only the ray comes from
// memory instead of the camera.  Nothing here may assume one origin for all rays: the per-frame octree table of
// render_kernel_oct, the v2 wave loop's origin-relative boxes and its bundle cull are not used.  The direction is taken as
// given (rayMarch does not normalise it).  Counts are exact u32: the reference's Uint16Array holds them mod 65536.
// PICK adds the object each ray hit; t, iters, sdf_calls and the normal do not depend on it (the object pass adds nothing to
// the count).  (Ahead-of-time only: the run-time specialiser's build of this file does not carry the ray queries.)
__device__ __forceinline__ Ray load_ray(const float *origins, const float *dirs, int64_t i) {
    Ray ray;
    ray.o = Vec3f{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]};
    ray.d = Vec3f{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    ray.od[0] = static_cast<double>(ray.o.x);  // per lane here (the camera's kernels take it from the parameter block)
    ray.od[1] = static_cast<double>(ray.o.y);
    ray.od[2] = static_cast<double>(ray.o.z);
    return ray;
}

template <int ACCEL, bool OTHER, int GEN, bool PICK>
__device__ __forceinline__ void query_body(const RmRenderParams &P, const float *origins, const float *dirs, int64_t n, int32_t want_normal,
                                           const int32_t *slot_obj, double *t_out, uint32_t *iters_out, uint32_t *sdf_out, float *normal_out,
                                           int32_t *obj_out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray ray = load_ray(origins, dirs, i);
    uint32_t count = 0, iters = 0;
    const double t = OTHER ? ray_march_other<ACCEL, GEN>(P, ray, count, iters) : ray_march<ACCEL, GEN>(P, ray, count, iters);
    Vec3f nrm{0.f, 0.f, 0.f};
    if (want_normal) nrm = hit_normal<ACCEL, GEN>(P, ray, t, count);
    if (t_out) t_out[i] = t;
    if (iters_out) iters_out[i] = iters;
    if (sdf_out) sdf_out[i] = count;
    if (normal_out) {
        normal_out[3 * i] = nrm.x;
        normal_out[3 * i + 1] = nrm.y;
        normal_out[3 * i + 2] = nrm.z;
    }
    if constexpr (PICK) {
        if (obj_out) obj_out[i] = hit_object<ACCEL, GEN>(P, ray, t, slot_obj);
    }
}

template <int ACCEL, bool OTHER, int GEN>
__global__ __launch_bounds__(256) void cast_kernel(const RmRenderParams P, const float *origins, const float *dirs, int64_t n, int32_t want_normal,
                                                   double *t_out, uint32_t *iters_out, uint32_t *sdf_out, float *normal_out) {
    query_body<ACCEL, OTHER, GEN, false>(P, origins, dirs, n, want_normal, nullptr, t_out, iters_out, sdf_out, normal_out, nullptr);
}

template <int ACCEL, bool OTHER, int GEN>
__global__ __launch_bounds__(256) void pick_kernel(const RmRenderParams P, const float *origins, const float *dirs, int64_t n, int32_t want_normal,
                                                   const int32_t *slot_obj, double *t_out, uint32_t *iters_out, uint32_t *sdf_out,
                                                   float *normal_out, int32_t *obj_out) {
    query_body<ACCEL, OTHER, GEN, true>(P, origins, dirs, n, want_normal, slot_obj, t_out, iters_out, sdf_out, normal_out, obj_out);
}

// ------------------------------------------------------------------ light queries (rm_ray_light)

// query_body's march and normal, then at hits the two light terms of include/rm_raymarch.h (rm_ray_light): one shadow ray
// towards the light through the SAME marcher and acceleration structure, and K Scene.getDistance samples along the normal.
// The marcher has one call site: trip 0 marches the caller's ray, trip 1 the shadow ray (a second inlined copy would double
// the kernel and its register pressure).  The lane's BVH hit-leaf list in LDS is dead once the primary march has returned
// (the marchers initialise it on entry), so the shadow ray reuses it.  Lanes whose ray missed, whose normal is zero or
// that face away from the light leave the loop after trip 0 and idle while the rest of the wave marches its shadow rays;
// lanes without a hit idle through the occlusion samples too.  That is accepted: the hit lanes of a wave of neighbouring
// rays are mostly the same, and compacting them would cost a pass through memory.
template <int ACCEL, bool OTHER, int GEN>
__device__ __forceinline__ void light_body(const RmRenderParams &P, const RmLightArgs &A) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    Ray ray = load_ray(A.origins, A.dirs, i);
    Vec3f p{0.f, 0.f, 0.f}, nrm{0.f, 0.f, 0.f};
    float lit = 1.f, ao = 1.f;
    uint32_t iters2 = 0, count2 = 0;
    bool hit = false;
#pragma unroll 1
    for (int trip = 0; trip < 2; ++trip) {
        uint32_t count = 0, iters = 0;
        const double t = OTHER ? ray_march_other<ACCEL, GEN>(P, ray, count, iters) : ray_march<ACCEL, GEN>(P, ray, count, iters);
        if (trip) {  // the shadow ray
            lit = t >= RM_MAX_DIST ? 1.f : 0.f;
            iters2 = iters;
            count2 = count;
            break;
        }
        nrm = hit_normal<ACCEL, GEN>(P, ray, t, count);
        if (A.t) A.t[i] = t;
        if (A.iters) A.iters[i] = iters;
        if (A.sdf) A.sdf[i] = count;
        if (A.normal) {
            A.normal[3 * i] = nrm.x;
            A.normal[3 * i + 1] = nrm.y;
            A.normal[3 * i + 2] = nrm.z;
        }
        if (t >= RM_MAX_DIST || (nrm.x == 0.f && nrm.y == 0.f && nrm.z == 0.f)) break;  // the neutral case
        hit = true;
        p.x = to_f32(static_cast<double>(ray.o.x) + static_cast<double>(ray.d.x) * t);  // hit_normal's point
        p.y = to_f32(static_cast<double>(ray.o.y) + static_cast<double>(ray.d.y) * t);
        p.z = to_f32(static_cast<double>(ray.o.z) + static_cast<double>(ray.d.z) * t);
        const double c = static_cast<double>(nrm.x) * A.light[0] + static_cast<double>(nrm.y) * A.light[1] + static_cast<double>(nrm.z) * A.light[2];
        if (!(c > 0.0)) {  // facing away (or NaN): dark, no shadow ray
            lit = 0.f;
            break;
        }
        ray.o.x = to_f32(static_cast<double>(p.x) + static_cast<double>(nrm.x) * A.bias);  // vec3.scaleAndAdd(p, n, bias)
        ray.o.y = to_f32(static_cast<double>(p.y) + static_cast<double>(nrm.y) * A.bias);
        ray.o.z = to_f32(static_cast<double>(p.z) + static_cast<double>(nrm.z) * A.bias);
        ray.d = Vec3f{A.light[0], A.light[1], A.light[2]};
        ray.od[0] = static_cast<double>(ray.o.x);
        ray.od[1] = static_cast<double>(ray.o.y);
        ray.od[2] = static_cast<double>(ray.o.z);
    }
    if (hit) {
        double occ = 0.0, w = 1.0;  // w = 2^(1 - k), exact
#pragma unroll 1
        for (int k = 1; k <= A.ao_samples; ++k) {
            const double h = static_cast<double>(k) * A.ao_step;
            Vec3f q;
            q.x = to_f32(static_cast<double>(p.x) + static_cast<double>(nrm.x) * h);
            q.y = to_f32(static_cast<double>(p.y) + static_cast<double>(nrm.y) * h);
            q.z = to_f32(static_cast<double>(p.z) + static_cast<double>(nrm.z) * h);
            const double d = scene_distance<ACCEL, GEN>(P, q, count2);
            occ = occ + (h - d) * w;
            w = w * 0.5;
        }
        const double x = 1.0 - A.ao_strength * occ;  // (K = 0: occ = 0 and x = 1)
        ao = to_f32(x > 0.0 ? (x > 1.0 ? 1.0 : x) : 0.0);  // NaN: 0
    }
    if (A.lit) A.lit[i] = lit;
    if (A.ao) A.ao[i] = ao;
    if (A.iters2) A.iters2[i] = iters2;
    if (A.sdf2) A.sdf2[i] = count2;
}

template <int ACCEL, bool OTHER, int GEN>
__global__ __launch_bounds__(256) void light_kernel(const RmRenderParams P, const RmLightArgs A) {
    light_body<ACCEL, OTHER, GEN>(P, A);
}

// ------------------------------------------------------------------ walk queries (rm_ray_walk)

// query_body's march (no normal) with a recorder: the summary of include/rm_raymarch.h (rm_walk) in registers and, when the
// launch wants traces (A.steps, the same for every lane), the first A.cap records of the ray at A.steps + i * A.cap.  The
// record index is all the recorder counts: EVAL records are the marcher's iters, the sum of their counts is its count, and
// the SKIP records are the rest.  A record leaves as plain stores (24 bytes at an 8-byte aligned address).
struct WalkRecorder {
    RmWalkStep *out;   // the ray's first slot, or null
    uint32_t cap, k;   // slots of the ray; records so far
    double min_dist, t_min, skipped;
    int end_reason;
    __device__ __forceinline__ void put(double t, double value, uint32_t n, int kind) {
        if (out && k < cap) {
            RmWalkStep s;
            s.t = t;
            s.value = value;
            s.count = n;
            s.kind = kind;
            out[k] = s;
        }
        k += 1;
    }
    __device__ __forceinline__ void eval(double t, double value, uint32_t n) {
        put(t, value, n, 0);
        if (value < min_dist) {  // (a NaN is never taken; the first record to reach the minimum keeps t_min)
            min_dist = value;
            t_min = t;
        }
    }
    __device__ __forceinline__ void skip(double t, double value) {
        put(t, value, 0, 1);
        skipped += value;
    }
    __device__ __forceinline__ void end(int reason) { end_reason = reason; }
};

template <int ACCEL, bool OTHER, int GEN>
__device__ __forceinline__ void walk_body(const RmRenderParams &P, const RmWalkArgs &A) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    Ray ray = load_ray(A.origins, A.dirs, i);
    WalkRecorder rec;
    rec.out = A.steps ? A.steps + i * A.cap : nullptr;
    rec.cap = static_cast<uint32_t>(A.cap);
    rec.k = 0;
    rec.min_dist = __builtin_inf();
    rec.t_min = 0.0;
    rec.skipped = 0.0;
    rec.end_reason = RM_WALK_STEPS;
    uint32_t count = 0, iters = 0;
    const double t = OTHER ? ray_march_other<ACCEL, GEN>(P, ray, count, iters, rec) : ray_march<ACCEL, GEN>(P, ray, count, iters, rec);
    if (A.walks) {
        RmWalkSummary w;
        w.t = t;
        w.min_dist = rec.min_dist;
        w.t_min = rec.t_min;
        w.skipped = rec.skipped;
        w.evals = iters;
        w.skips = rec.k - iters;
        w.sdf_calls = count;
        w.end = rec.end_reason;
        A.walks[i] = w;
    }
}

template <int ACCEL, bool OTHER, int GEN>
__global__ __launch_bounds__(256) void walk_kernel(const RmRenderParams P, const RmWalkArgs A) {
    walk_body<ACCEL, OTHER, GEN>(P, A);
}

#ifndef RM_LENGTH_SQRT
__global__ __launch_bounds__(256) void hypot_kernel(const float *xyz, int64_t n, double *out) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    out[i] = hypot3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}

// hypot3 (compiler's IEEE division) vs hypot3_shared_rcp on counter-generated binary32
// triples: random mantissas, exponents spread over [2^-149, 2^60], zeros, equal and
// near-equal magnitudes.  Counts bitwise mismatches.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ float gen_f32(uint64_t r, int mode) {
    const uint32_t mant = static_cast<uint32_t>(r) & 0x7FFFFFu;
    const uint32_t sign = static_cast<uint32_t>(r >> 63) << 31;
    uint32_t exp;
    const uint32_t sel = static_cast<uint32_t>(r >> 40) & 0xFFu;
    if (mode == 0) exp = 96 + sel % 64;        // around 1: 2^-31 .. 2^32
    else if (mode == 1) exp = sel % 188;       // whole low range incl. denormals (exp 0)
    else exp = 120 + sel % 10;                 // same binade neighbourhood
    if ((r >> 50 & 0x3F) == 0) return __uint_as_float(sign);  // +-0
    return __uint_as_float(sign | (exp << 23) | mant);
}

__global__ __launch_bounds__(256) void fastdiv_selftest_kernel(uint64_t seed, int64_t n, unsigned long long *mismatches) {
    unsigned long long bad = 0;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const uint64_t base = seed + 3ull * static_cast<uint64_t>(i);
        const int mode = static_cast<int>(i % 3);
        float a = gen_f32(mix64(base), mode), b = gen_f32(mix64(base + 1), mode), c = gen_f32(mix64(base + 2), mode);
        if ((i & 15) == 7) b = a;                     // equal magnitudes: quotient exactly 1
        if ((i & 31) == 19) c = -a;
        if ((i & 63) == 33) b = __uint_as_float(__float_as_uint(a) + 1);  // one ulp apart
        const double x = hypot3(a, b, c), y = hypot3_shared_rcp(a, b, c);
        if (__double_as_longlong(x) != __double_as_longlong(y)) bad++;
    }
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(mismatches, bad);
}

// mode 0: 1.0 / d for every finite non-zero binary32 d (2^32 bit patterns); mode 1: x / W for 0 <= x < 2^16, 1 <= W < 2^16
__global__ __launch_bounds__(256) void recip_selftest_kernel(int mode, unsigned long long *mismatches) {
    unsigned long long bad = 0;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < (1ull << 32);
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        double a, b;
        if (mode == 0) {
            const float d = __uint_as_float(static_cast<uint32_t>(i));
            if (!(__builtin_fabsf(d) <= 3.4028234663852886e38f) || d == 0.0f) continue;
            a = 1.0;
            b = static_cast<double>(d);
        } else {
            const uint32_t x = static_cast<uint32_t>(i >> 16), w = static_cast<uint32_t>(i & 0xFFFFu);
            if (w == 0) continue;
            a = static_cast<double>(x);
            b = static_cast<double>(w);
        }
        // opaque to the optimiser, so that the reference quotient is the compiler's full IEEE expansion
        asm volatile("" : "+v"(a), "+v"(b));
        const double want = a / b, got = div_in_range(a, b);
        if (__double_as_longlong(want) != __double_as_longlong(got)) bad++;
    }
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(mismatches, bad);
}

#endif  // !RM_LENGTH_SQRT

}  // namespace

#ifndef RM_LENGTH_SQRT
hipError_t rm_launch_recip_selftest(int mode, unsigned long long *d_mismatches, hipStream_t stream) {
    hipLaunchKernelGGL(recip_selftest_kernel, dim3(4096), dim3(256), 0, stream, mode, d_mismatches);
    return hipGetLastError();
}

hipError_t rm_launch_fastdiv_selftest(uint64_t seed, int64_t n, unsigned long long *d_mismatches, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fastdiv_selftest_kernel, dim3(2048), dim3(256), 0, stream, seed, n, d_mismatches);
    return hipGetLastError();
}

#endif  // !RM_LENGTH_SQRT

// ---------------------------------------------------------------------- launchers

namespace {
// The dynamic LDS of a one-ray-per-lane launch of `threads` lanes: the expression programs' position slots and pending
// values (rm_program.h), then, 16-byte aligned behind them, the per-ray BVH hit-leaf lists (v1_lists_begin reads
// v1_list_offset; -1: no lists) -- where the caller wants them, the scene has them and they fit.
struct V1Lds {
    size_t bytes;
    int32_t v1_list_offset;
};
V1Lds v1_lds_layout(const RmRenderParams &p, int threads, bool lists) {
    V1Lds l{p.general >= 2 ? (static_cast<size_t>(p.prog_slots) * 12 + static_cast<size_t>(p.prog_vals) * 8) * threads : 0, -1};
    const size_t list_bytes = static_cast<size_t>(2) * RM_V1_LIST_CAP * threads;
    if (lists && p.accel == 2 && p.v1_lists && p.general < 2 && p.bvh_nodes < 65536 && l.bytes + list_bytes <= 64 * 1024) {
        l.v1_list_offset = static_cast<int32_t>((l.bytes + 15) & ~static_cast<size_t>(15));
        l.bytes = static_cast<size_t>(l.v1_list_offset) + list_bytes;
    }
    return l;
}

// What the launch of a ray query is, whichever kernel it names: nothing without a ray (grid.x 0), else one lane per ray in
// 256-thread workgroups, the LDS of the one-ray-per-lane render launch -- so every march of a lane is a render's -- and the
// parameter block without a run-time specialised kernel (the ray queries are ahead-of-time only) or diagnostics.
struct RayLaunch {
    dim3 grid, block;
    size_t shmem;
    RmRenderParams pl;
};
RayLaunch ray_launch(const RmRenderParams &p, long long n) {
    const int threads = 256;
    const V1Lds lds = v1_lds_layout(p, threads, true);
    RayLaunch l{dim3(n > 0 ? static_cast<unsigned>((n + threads - 1) / threads) : 0u), dim3(threads), lds.bytes, p};
    l.pl.rtc_function = nullptr;
    l.pl.diag_block = nullptr;
    l.pl.diag_out = nullptr;
    l.pl.v1_list_offset = lds.v1_list_offset;
    return l;
}
// What the launch of a query without a ray is (field, blocks, tiles, points, sharp vertices), whichever kernel it names: the
// dynamic LDS of a 256-thread workgroup without hit-leaf lists -- a point has no ray -- and the parameter block without a
// run-time specialised kernel or diagnostics.  The grid is the launcher's: each family counts its workgroups its own way.
struct SceneLaunch {
    size_t shmem;
    RmRenderParams pl;
};
SceneLaunch scene_launch(const RmRenderParams &p) {
    SceneLaunch l{v1_lds_layout(p, 256, false).bytes, p};
    l.pl.rtc_function = nullptr;
    l.pl.diag_block = nullptr;
    l.pl.diag_out = nullptr;
    return l;
}
}  // namespace

// RM_DISPATCH(K): K(ACCEL, OTHER, GEN) for the instantiation the parameter block `p` in scope selects (accel, algorithm, general).
#define RM_DISPATCH_A(K, O, G) { if (p.accel == 2) K(2, O, G) else if (p.accel == 1) K(1, O, G) else K(0, O, G) }
#define RM_DISPATCH_O(K, G) { if (p.algorithm == 0) RM_DISPATCH_A(K, false, G) else RM_DISPATCH_A(K, true, G) }
#define RM_DISPATCH(K) { if (p.general == 3) RM_DISPATCH_O(K, 3) else if (p.general == 2) RM_DISPATCH_O(K, 2) else if (p.general) RM_DISPATCH_O(K, 1) else RM_DISPATCH_O(K, 0) }
#define RM_KERNEL_NAME(kernel, A, O, G) #kernel "<" #A ", " #O ", " #G ">" RM_LEN_TAG
// The point, field, tile and sharp-vertex launches of option `exact` (p.accel == RM_ACCEL_EXACT), with grid, block, the
// SceneLaunch `l`, stream and kernel_name in scope: exact_kernel<GEN> for sphere and primitive records; expression programs have
// no tree to walk and run kernel<0, GEN>, which evaluates every object.  rm_last_kernel reports "kernel<EXACT, GEN>" for all of them.
#define RM_EXACT_ONE(label, KERNEL, G, ...)                                          \
    {                                                                                \
        hipLaunchKernelGGL(KERNEL, grid, block, l.shmem, stream, __VA_ARGS__);       \
        if (kernel_name) *kernel_name = label "<EXACT, " #G ">" RM_LEN_TAG;          \
    }
#define RM_LAUNCH_EXACT(kernel, exact_kernel, ...)                                                 \
    {                                                                                              \
        if (p.general == 3) RM_EXACT_ONE(#kernel, (kernel<0, 3>), 3, __VA_ARGS__)                  \
        else if (p.general == 2) RM_EXACT_ONE(#kernel, (kernel<0, 2>), 2, __VA_ARGS__)             \
        else if (p.general) RM_EXACT_ONE(#kernel, (exact_kernel<1>), 1, __VA_ARGS__)               \
        else RM_EXACT_ONE(#kernel, (exact_kernel<0>), 0, __VA_ARGS__)                              \
    }

hipError_t RM_LEN_VARIANT(rm_launch_render)(const RmRenderParams &p, hipStream_t stream, const char **kernel_name, uint32_t *v2_shape) {
    const int rows = p.local_rows;
    if (kernel_name) *kernel_name = "";
    if (rows <= 0 || p.width <= 0) return hipSuccess;
    if (p.variant == 2 && p.algorithm == 0) return RM_LEN_VARIANT(rm_launch_render_v2)(p, stream, kernel_name, v2_shape);
    const int tw = p.tile_w, th = 64 / tw;
    const int wpw = p.v1_block >= 256 ? 4 : (p.v1_block >= 128 ? 2 : 1);  // waves per workgroup (option `v1_block`)
    const int threads = 64 * wpw;
    const int tiles_x = (p.width + tw - 1) / tw;
    const int tiles_y = (rows + wpw * th - 1) / (wpw * th);
    const dim3 grid((static_cast<unsigned>(tiles_x) * static_cast<unsigned>(tiles_y) + 63u) & ~63u), block(static_cast<unsigned>(threads));  // v1_tile_of_block
    const V1Lds lds = p.rtc_function ? V1Lds{0, -1} : v1_lds_layout(p, threads, true);
    const size_t shmem = lds.bytes;
    RmRenderParams pl = p;
    pl.v1_list_offset = lds.v1_list_offset;
    if (p.rtc_function) {  // this scene's run-time specialised kernel (rm_rtc.h): same grid, nothing in LDS (set by the API layer for these launches only)
        size_t bytes = sizeof pl;
        void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &pl, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
        return hipModuleLaunchKernel(reinterpret_cast<hipFunction_t>(const_cast<void *>(p.rtc_function)), grid.x, 1, 1, block.x, 1, 1, 0, stream, nullptr,
                                     extra);
    }
#define RM_V1(A, O, G)                                                               \
    {                                                                                \
        hipLaunchKernelGGL((render_kernel<A, O, G>), grid, block, shmem, stream, pl); \
        if (kernel_name) *kernel_name = RM_KERNEL_NAME(render_kernel, A, O, G);      \
    }
    if (p.accel == 1 && p.general == 0 && p.algorithm == 0 && p.oct_lean && p.oct_frame && p.oct_lut && p.oct_recs && p.filter && p.oct_nodes < (1 << 24) &&
        p.oct_prim_count < (1 << 26)) {  // 32-bit byte offsets into the node and record tables
        // one wave per workgroup, 8 x 8 pixels: wave slots refill one by one (four-wave workgroups wait for a free slot on every
        // SIMD: 3.10 -> 2.89 ms on the 10 000-sphere frame), and a square tile keeps the rays of a wave in the same leaves
        pl.tile_w = 8;
        const int ty = (rows + 7) / 8;
        hipLaunchKernelGGL(render_kernel_oct, dim3((static_cast<unsigned>((p.width + 7) / 8) * static_cast<unsigned>(ty) + 63u) & ~63u), dim3(64), 0, stream,
                           pl);  // the lean octree sphere tracer (finite camera: rm_api.cpp)
        if (kernel_name) *kernel_name = "render_kernel_oct" RM_LEN_TAG;
    } else RM_DISPATCH(RM_V1)
#undef RM_V1
    return hipGetLastError();
}

// n_views frames of rows [y_start, y_end) in one launch: the grid of a one-ray-per-lane render launch (tile_w, v1_block) in x, the
// frame in y (n_views <= 65535).  Ahead-of-time kernels only, the general ones (no lean octree kernel: its table is per camera).
hipError_t RM_LEN_VARIANT(rm_launch_frames)(const RmRenderParams &p, const RmFrameView *views, int32_t n_views, RmFrameDiagBlock *blocks,
                                            RmDiagDevice *acc, hipStream_t stream, const char **kernel_name) {
    const int rows = p.local_rows;
    if (kernel_name) *kernel_name = "";
    if (n_views <= 0) return hipSuccess;
    if (rows <= 0 || p.width <= 0) {
#ifdef RM_LENGTH_SQRT
        return rm_launch_frames(p, views, n_views, blocks, acc, stream, kernel_name);
#else
        if (acc) hipLaunchKernelGGL(frames_neutral_kernel, dim3(static_cast<unsigned>((n_views + 255) / 256)), dim3(256), 0, stream, acc, n_views);
        return hipGetLastError();
#endif
    }
    const int tw = p.tile_w, th = 64 / tw;
    const int wpw = p.v1_block >= 256 ? 4 : (p.v1_block >= 128 ? 2 : 1);
    const int threads = 64 * wpw;
    const int tiles_x = (p.width + tw - 1) / tw;
    const int tiles_y = (rows + wpw * th - 1) / (wpw * th);
    const dim3 grid((static_cast<unsigned>(tiles_x) * static_cast<unsigned>(tiles_y) + 63u) & ~63u, static_cast<unsigned>(n_views)),
        block(static_cast<unsigned>(threads));  // x: v1_tile_of_block
    const V1Lds lds = v1_lds_layout(p, threads, true);
    const size_t shmem = lds.bytes;
    RmRenderParams pl = p;
    pl.rtc_function = nullptr;
    pl.oct_frame = nullptr;
    pl.diag_block = nullptr;
    pl.diag_out = nullptr;
    pl.v1_list_offset = lds.v1_list_offset;
#define RM_FK(A, O, G)                                                                                   \
    {                                                                                                    \
        hipLaunchKernelGGL((frames_kernel<A, O, G>), grid, block, shmem, stream, pl, views, blocks, acc); \
        if (kernel_name) *kernel_name = RM_KERNEL_NAME(frames_kernel, A, O, G);                          \
    }
    RM_DISPATCH(RM_FK)
#undef RM_FK
    return hipGetLastError();
}

#ifndef RM_LENGTH_SQRT
hipError_t rm_launch_oct_frame_table(const RmOctNode *nodes, int n, const double origin[3], RmOctFrameNode *out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(oct_frame_table_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, nodes, n, origin[0], origin[1],
                       origin[2], out);
    return hipGetLastError();
}

hipError_t rm_launch_shade(int shader, int64_t n, const uint8_t *depth, const uint8_t *normal, const uint16_t *sdf,
                           const uint16_t *iters, uint8_t *rgba, const float light[3], hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(shade_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, shader, n, depth,
                       normal, sdf, iters, reinterpret_cast<uchar4 *>(rgba), light[0], light[1], light[2]);
    return hipGetLastError();
}

hipError_t rm_launch_reduce_init(RmDiagDevice *acc, hipStream_t stream) {
    hipLaunchKernelGGL(reduce_init_kernel, dim3(1), dim3(1), 0, stream, acc);
    return hipGetLastError();
}

hipError_t rm_launch_reduce(const uint16_t *sdf, const uint16_t *iters, int64_t n, RmDiagDevice *acc,
                            hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n / 8 + 255) / 256;
    if (blocks > 128) blocks = 128;  // one atomic set per workgroup on one cache line: they serialise (256 workgroups: 17.6 us for init +
                                     // reduce of a 4K frame, 128: 12.6 us, of which two launches are ~12; 64 x 1024 threads: 12.0 us)
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(reduce_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, sdf, iters, n, acc);
    return hipGetLastError();
}

#endif  // !RM_LENGTH_SQRT

hipError_t RM_LEN_VARIANT(rm_launch_distance)(const RmRenderParams &p, const float *points, int64_t n, double *dist, uint32_t *count,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    const size_t shmem = scene_launch(p).shmem;  // (its LDS only: this launch keeps p.rtc_function, the branch below)
    if (p.rtc_function) {  // rm_rtc_distance(RmRenderParams, const float *, int64_t, double *, uint32_t *)
        struct Args {
            RmRenderParams p;
            const float *points;
            int64_t n;
            double *dist;
            uint32_t *count;
        } args{p, points, n, dist, count};
        static_assert(sizeof(RmRenderParams) % 8 == 0 && alignof(RmRenderParams) == 8, "kernel argument layout");
        size_t bytes = sizeof args;
        void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
        return hipModuleLaunchKernel(reinterpret_cast<hipFunction_t>(const_cast<void *>(p.rtc_function)), grid.x, 1, 1, 256, 1, 1, 0, stream, nullptr, extra);
    }
#define RM_DK(A, O, G) { hipLaunchKernelGGL((distance_kernel<A, G>), grid, block, shmem, stream, p, points, n, dist, count); }
    RM_DISPATCH(RM_DK)
#undef RM_DK
    return hipGetLastError();
}

hipError_t RM_LEN_VARIANT(rm_launch_field)(const RmRenderParams &p, const RmFieldArgs &a, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "";
    if (a.n <= 0 || a.nu == 0 || a.nv == 0) return hipSuccess;
    const SceneLaunch l = scene_launch(p);
    RmFieldArgs al = a;
    const long long blocks = (a.n + 255) / 256;
    for (long long done = 0; done < blocks; done += 1ll << 22) {  // one grid dimension: at most 2^22 workgroups (2^30 points) a launch
        const long long m = blocks - done < (1ll << 22) ? blocks - done : (1ll << 22);
        const dim3 grid(static_cast<unsigned>(m)), block(256);
        al.block_first = done;
#define RM_FLDK(A, O, G)                                                                    \
    {                                                                                       \
        hipLaunchKernelGGL((field_kernel<A, G>), grid, block, l.shmem, stream, l.pl, al);   \
        if (kernel_name) *kernel_name = "field_kernel<" #A ", " #G ">" RM_LEN_TAG;          \
    }
        if (p.accel == RM_ACCEL_EXACT) RM_LAUNCH_EXACT(field_kernel, field_exact_kernel, l.pl, al)
        else RM_DISPATCH(RM_FLDK)
#undef RM_FLDK
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t RM_LEN_VARIANT(rm_launch_blocks)(const RmRenderParams &p, const RmBlocksArgs &a, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "";
    if (a.n_blocks == 0 || a.n_blocks > RM_SPARSE_MAX_BLOCKS || a.n_groups != (a.n_blocks + 255u) / 256u) return hipErrorInvalidValue;
    const SceneLaunch l = scene_launch(p);
    const dim3 grid(a.n_groups), block(256);
    // the pruned walk where there is a tree of boxes around sphere or primitive records; every object otherwise
    const bool walk = p.accel == 2 && p.general < 2 && p.bvh_nodes > 0;
#define RM_BLK(G, W)                                                                   \
    {                                                                                  \
        hipLaunchKernelGGL((blocks_kernel<G, W>), grid, block, l.shmem, stream, l.pl, a); \
        if (kernel_name) *kernel_name = "blocks_kernel<" #G ", " #W ">" RM_LEN_TAG;    \
    }
    if (p.general == 3) RM_BLK(3, false)
    else if (p.general == 2) RM_BLK(2, false)
    else if (p.general) {
        if (walk) RM_BLK(1, true) else RM_BLK(1, false)
    } else {
        if (walk) RM_BLK(0, true) else RM_BLK(0, false)
    }
#undef RM_BLK
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rm_launch_blocks_compact(a, stream);
}

hipError_t RM_LEN_VARIANT(rm_launch_tiles)(const RmRenderParams &p, const RmTilesArgs &a, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "";
    if (a.n_kept == 0 || a.n_kept > RM_SPARSE_MAX_BLOCKS) return hipErrorInvalidValue;
    const SceneLaunch l = scene_launch(p);
    const dim3 grid(a.n_kept), block(256);
#define RM_TLK(A, O, G)                                                                  \
    {                                                                                    \
        hipLaunchKernelGGL((tiles_kernel<A, G>), grid, block, l.shmem, stream, l.pl, a); \
        if (kernel_name) *kernel_name = "tiles_kernel<" #A ", " #G ">" RM_LEN_TAG;       \
    }
    if (p.accel == RM_ACCEL_EXACT) RM_LAUNCH_EXACT(tiles_kernel, tiles_exact_kernel, l.pl, a)
    else RM_DISPATCH(RM_TLK)
#undef RM_TLK
    return hipGetLastError();
}

hipError_t RM_LEN_VARIANT(rm_launch_tiles_update)(const RmRenderParams &p, const RmTilesArgs &a, const RmTilesUpdateArgs &u, hipStream_t stream,
                                                  const char **kernel_name) {
    if (kernel_name) *kernel_name = "";
    if (a.n_kept == 0 || a.n_kept > RM_SPARSE_MAX_BLOCKS || u.n_balls < 0 || u.n_balls > RM_UPDATE_MAX_BALLS) return hipErrorInvalidValue;
    if (p.accel != RM_ACCEL_EXACT || p.general >= 2) return hipErrorInvalidValue;  // (expression programs: the full path)
    const SceneLaunch l = scene_launch(p);
    const dim3 grid(a.n_kept), block(256);
    if (p.general) {
        hipLaunchKernelGGL((tiles_update_kernel<1>), grid, block, l.shmem, stream, l.pl, a, u);
        if (kernel_name) *kernel_name = "tiles_update_kernel<1>" RM_LEN_TAG;
    } else {
        hipLaunchKernelGGL((tiles_update_kernel<0>), grid, block, l.shmem, stream, l.pl, a, u);
        if (kernel_name) *kernel_name = "tiles_update_kernel<0>" RM_LEN_TAG;
    }
    return hipGetLastError();
}

hipError_t RM_LEN_VARIANT(rm_launch_points)(const RmRenderParams &p, const RmPointArgs &a, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "";
    if (a.n <= 0) return hipSuccess;
    const SceneLaunch l = scene_launch(p);
    const dim3 grid(static_cast<unsigned>((a.n + 255) / 256)), block(256);  // (a.n <= INT32_MAX: one grid dimension)
#define RM_PTK(A, O, G)                                                                  \
    {                                                                                    \
        hipLaunchKernelGGL((point_kernel<A, G>), grid, block, l.shmem, stream, l.pl, a); \
        if (kernel_name) *kernel_name = "point_kernel<" #A ", " #G ">" RM_LEN_TAG;       \
    }
    if (p.accel == RM_ACCEL_EXACT) RM_LAUNCH_EXACT(point_kernel, point_exact_kernel, l.pl, a)
    else RM_DISPATCH(RM_PTK)
#undef RM_PTK
    return hipGetLastError();
}

hipError_t RM_LEN_VARIANT(rm_launch_sharp)(const RmRenderParams &p, const RmSharpArgs &a, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "";
    if (a.n <= 0) return hipSuccess;
    if (a.refine < 0 || a.refine > 8) return hipErrorInvalidValue;
    const SceneLaunch l = scene_launch(p);
    const dim3 grid(static_cast<unsigned>((a.n + RM_SHARP_CELLS - 1) / RM_SHARP_CELLS)), block(256);  // (a.n <= INT32_MAX: one grid dimension)
#define RM_SHK(A, O, G)                                                                  \
    {                                                                                    \
        hipLaunchKernelGGL((sharp_kernel<A, G>), grid, block, l.shmem, stream, l.pl, a); \
        if (kernel_name) *kernel_name = "sharp_kernel<" #A ", " #G ">" RM_LEN_TAG;       \
    }
    if (p.accel == RM_ACCEL_EXACT) RM_LAUNCH_EXACT(sharp_kernel, sharp_kernel_exact, l.pl, a)
    else RM_DISPATCH(RM_SHK)
#undef RM_SHK
    return hipGetLastError();
}

// The ray queries (ray_launch, above).  What is left per family: the line that names its kernel and hands it its arguments
// where the kernel reads them (RmRays `r`, the block `a`, RayLaunch `l`, `stream` and `kernel_name` in scope).
#define RM_RAY_K(kernel, A, O, G, ...)                                                              \
    {                                                                                               \
        hipLaunchKernelGGL((kernel<A, O, G>), l.grid, l.block, l.shmem, stream, l.pl, __VA_ARGS__); \
        if (kernel_name) *kernel_name = RM_KERNEL_NAME(kernel, A, O, G);                            \
    }
#define RM_CK(A, O, G) RM_RAY_K(cast_kernel, A, O, G, r.origins, r.dirs, static_cast<int64_t>(r.n), a.want_normal, a.t, a.iters, a.sdf, a.normal)
#define RM_PK(A, O, G) RM_RAY_K(pick_kernel, A, O, G, r.origins, r.dirs, static_cast<int64_t>(r.n), a.want_normal, a.slot_obj, a.t, a.iters, a.sdf, a.normal, a.object)
#define RM_LK(A, O, G) RM_RAY_K(light_kernel, A, O, G, al)
#define RM_WK(A, O, G) RM_RAY_K(walk_kernel, A, O, G, al)

hipError_t RM_LEN_VARIANT(rm_launch_cast)(const RmRenderParams &p, const RmRays &r, const RmQueryArgs &a, hipStream_t stream, const char **kernel_name) {
    const RayLaunch l = ray_launch(p, r.n);
    if (kernel_name) *kernel_name = "";
    if (!l.grid.x) return hipSuccess;
    RM_DISPATCH(RM_CK)
    return hipGetLastError();
}
hipError_t RM_LEN_VARIANT(rm_launch_pick)(const RmRenderParams &p, const RmRays &r, const RmQueryArgs &a, hipStream_t stream, const char **kernel_name) {
    const RayLaunch l = ray_launch(p, r.n);
    if (kernel_name) *kernel_name = "";
    if (!l.grid.x) return hipSuccess;
    RM_DISPATCH(RM_PK)
    return hipGetLastError();
}
hipError_t RM_LEN_VARIANT(rm_launch_light)(const RmRenderParams &p, const RmRays &r, const RmLightArgs &a, hipStream_t stream, const char **kernel_name) {
    const RayLaunch l = ray_launch(p, r.n);
    if (kernel_name) *kernel_name = "";
    if (!l.grid.x) return hipSuccess;
    RmLightArgs al = a;
    al.origins = r.origins;
    al.dirs = r.dirs;
    al.n = r.n;
    RM_DISPATCH(RM_LK)
    return hipGetLastError();
}
hipError_t RM_LEN_VARIANT(rm_launch_walk)(const RmRenderParams &p, const RmRays &r, const RmWalkArgs &a, hipStream_t stream, const char **kernel_name) {
    const RayLaunch l = ray_launch(p, r.n);
    if (kernel_name) *kernel_name = "";
    if (!l.grid.x) return hipSuccess;
    RmWalkArgs al = a;
    al.origins = r.origins;
    al.dirs = r.dirs;
    al.n = r.n;
    RM_DISPATCH(RM_WK)
    return hipGetLastError();
}
#undef RM_WK
#undef RM_LK
#undef RM_PK
#undef RM_CK
#undef RM_RAY_K

#ifndef RM_LENGTH_SQRT
__global__ __launch_bounds__(256) void jsmath_kernel(int fn, const double *a, const double *b, int64_t n, double *out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b[i];
    double r;
    switch (fn) {
        case 0: r = js_sin(x); break;
        case 1: r = js_cos(x); break;
        case 2: r = js_atan2(x, y); break;
        case 3: r = js_asin(x); break;
        case 4: r = js_log(x); break;
        case 5: r = js_pow(x, y); break;
        case 6: r = js_round(x); break;
        default: r = js_atan(x); break;
    }
    out[i] = r;
}

hipError_t rm_launch_jsmath(int fn, const double *a, const double *b, int64_t n, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(jsmath_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, fn, a, b, n, out);
    return hipGetLastError();
}

hipError_t rm_launch_hypot(const float *xyz, int64_t n, double *out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(hypot_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, xyz, n, out);
    return hipGetLastError();
}
#endif  // !RM_LENGTH_SQRT
#endif  // !RM_RTC
