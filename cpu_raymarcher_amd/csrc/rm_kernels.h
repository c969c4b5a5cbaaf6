// rm_kernels.h -- launchers of the gfx950 kernels in rm_kernels.hip.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#endif

#include "rm_types.h"

struct RmDiagDevice {  // accumulator of rm_reduce_counters_device (32 bytes)
    unsigned long long total_sdf;
    unsigned long long total_iters;
    unsigned int max_sdf;
    unsigned int min_sdf;
    unsigned long long pad;
};

// rm_kernels.hip and rm_render_v2.hip are compiled twice: as they are (vec3.length = Math.hypot, the gl-matrix 3.0 -
// 3.4.3 form) and with -DRM_LENGTH_SQRT (vec3.length = Math.sqrt(x*x + y*y + z*z); entry points carry the suffix
// _sqrt).  Option `length` picks the set (rm_device.h, vec3_length).
#ifdef RM_LENGTH_SQRT
#define RM_LEN_VARIANT(name) name##_sqrt
#define RM_LEN_TAG " [length=sqrt]"
#define RM_LEN_IS_SQRT true
#else
#define RM_LEN_VARIANT(name) name
#define RM_LEN_TAG ""
#define RM_LEN_IS_SQRT false
#endif

// The screen rectangle of a leaf box under a launch's camera (RmLeafRect; option `rect_cull`): one text for the wave loop,
// which fills the launch's table with it, and for rm_debug_leaf_rects, which needs no device.  make_ray sends pixel (x, y) of
// the W x H frame along d = u c0 + v c1 - c2 with u = (x / W - 0.5) * 2, v = (y / H - 0.5) * 2 and c0, c1, c2 the columns of
// `rot`.  With orthonormal columns a point q = s d (s >= 0) of that ray, taken from the camera position, has -q.c2 = s and
// q.c0 = s u, q.c1 = s v: the ray passes through a box only if (u, v) lies in the box's image under q -> (q.c0, q.c1) / z,
// z = -q.c2.  Where z > 0 on all of the box, each coordinate is a ratio of linear functions with a positive denominator, which
// takes its extremes over a box at corners: the image lies in [min u, max u] x [min v, max v] over the eight corners.
//   * binary64 throughout; host and device compile it without contraction, so both give the same table;
//   * a corner with z at or below 1e-6 of its own L1 norm (at or behind the camera plane, or NaN) gives the whole frame;
//   * the rectangle is widened by what the plane cull widens its bundle by, half a pixel spacing max(1 / W, 1e-4) -- a
//     thousand times the rounding of a ray direction to binary32 and of the columns' departure from orthonormal that
//     rm_rect_cull_camera_ok admits (each moves u by less than 1e-5 inside the frame) -- plus 1e-6 (1 + |u|) for this function's own roundings;
//   * pixel bounds are rounded outwards and clamped to 0 .. 65535: W, H <= 65536 is the caller's to check;
//   * a rectangle that misses the frame on one side holds no pixel; anything non-finite gives the whole frame.
inline __host__ __device__ RmLeafRect rm_leaf_rect(const float lo[3], const float hi[3], const float o[3], const float rot[9], int W, int H) {
    const RmLeafRect whole = {0, 65535, 0, 65535}, none = {65535, 0, 65535, 0};
    double ql[3], qh[3];
    for (int k = 0; k < 3; ++k) {
        ql[k] = static_cast<double>(lo[k]) - static_cast<double>(o[k]);
        qh[k] = static_cast<double>(hi[k]) - static_cast<double>(o[k]);
    }
    double umin = 0.0, umax = 0.0, vmin = 0.0, vmax = 0.0;
    bool behind = false;
#pragma unroll 1  // (in the wave loop's kernel: eight corners side by side, two divisions each, would want more registers than it has)
    for (int corner = 0; corner < 8; ++corner) {
        const double qx = (corner & 1) ? qh[0] : ql[0], qy = (corner & 2) ? qh[1] : ql[1], qz = (corner & 4) ? qh[2] : ql[2];
        const double z = -(qx * rot[6] + qy * rot[7] + qz * rot[8]);
        const double a = qx * rot[0] + qy * rot[1] + qz * rot[2];
        const double b = qx * rot[3] + qy * rot[4] + qz * rot[5];
        if (!(z > 1e-6 * (__builtin_fabs(qx) + __builtin_fabs(qy) + __builtin_fabs(qz)))) behind = true;
        const double u = a / z, v = b / z;
        if (corner == 0 || u < umin) umin = u;
        if (corner == 0 || u > umax) umax = u;
        if (corner == 0 || v < vmin) vmin = v;
        if (corner == 0 || v > vmax) vmax = v;
    }
    if (behind) return whole;
    const double mu = __builtin_fmax(1.0 / W, 1e-4), mv = __builtin_fmax(1.0 / H, 1e-4);
    // pixel x has u = (x / W - 0.5) * 2: x = (u / 2 + 0.5) W
    const double xl = ((umin - mu - 1e-6 * (1.0 + __builtin_fabs(umin))) * 0.5 + 0.5) * W;
    const double xh = ((umax + mu + 1e-6 * (1.0 + __builtin_fabs(umax))) * 0.5 + 0.5) * W;
    const double yl = ((vmin - mv - 1e-6 * (1.0 + __builtin_fabs(vmin))) * 0.5 + 0.5) * H;
    const double yh = ((vmax + mv + 1e-6 * (1.0 + __builtin_fabs(vmax))) * 0.5 + 0.5) * H;
    if (!(xl - xl == 0.0 && xh - xh == 0.0 && yl - yl == 0.0 && yh - yh == 0.0)) return whole;  // an infinity or a NaN
    if (xh < 0.0 || yh < 0.0 || xl > W - 1.0 || yl > H - 1.0) return none;
    RmLeafRect r;
    r.x_lo = static_cast<uint16_t>(xl <= 0.0 ? 0 : (xl >= 65535.0 ? 65535 : static_cast<int>(__builtin_floor(xl))));
    r.x_hi = static_cast<uint16_t>(xh >= 65535.0 ? 65535 : static_cast<int>(__builtin_ceil(xh)));
    r.y_lo = static_cast<uint16_t>(yl <= 0.0 ? 0 : (yl >= 65535.0 ? 65535 : static_cast<int>(__builtin_floor(yl))));
    r.y_hi = static_cast<uint16_t>(yh >= 65535.0 ? 65535 : static_cast<int>(__builtin_ceil(yh)));
    return r;
}

// The order keys of the one-radius scan (rm_render_v2.hip scan_sphere<true>: a sphere's squared centre distance, its id in the
// low byte) and the three smallest of them: one text for the wave loop and for rm_debug_scan_keys, which needs no device.
// All three start at all ones ("no sphere").  After any number of updates best <= second <= third are the three smallest keys
// fed so far, equal keys counted as often as they came -- five integer min / max, no compare and no select:
//   lo = min(best, key), hi = max(best, key): the new best, and whichever of the two is displaced;
//   mid = max(second, hi): whichever of those two is displaced in turn (taken before second changes);
//   second = min(second, hi);  third = min(third, mid).
// Section M's runner-up test (option `runner_up`) reads the second key's id and the third key's distance.
struct RmScanKeys {
    uint32_t best, second, third;
};
inline __host__ __device__ void rm_scan_keys_update(RmScanKeys &k, uint32_t key) {
    const uint32_t lo = key < k.best ? key : k.best, hi = key < k.best ? k.best : key;
    const uint32_t mid = hi < k.second ? k.second : hi;
    k.best = lo;
    k.second = hi < k.second ? hi : k.second;
    k.third = mid < k.third ? mid : k.third;
}
// the key of a squared distance s2 >= 0 (its bit pattern, which orders like the value) and a sphere id below 256
inline __host__ __device__ uint32_t rm_scan_key(uint32_t s2_bits, uint32_t id) { return (s2_bits & 0xFFFFFF00u) | (id & 0xFFu); }
// A key's conservative binary32 lower bound of that sphere's distance (radius rf), by the formula and margin of
// scan_finish_uniform (rm_render_v2.hip); +inf for the all-ones key: there is no such sphere.  Clearing the id byte only lowers
// s2, and the bound is monotone in s2 up to what the margin absorbs, so it bounds every sphere whose key is no smaller.
inline __host__ __device__ float rm_scan_key_bound(uint32_t key, float rf) {
    const float s2 = __builtin_bit_cast(float, key & 0xFFFFFF00u);
#ifdef __HIP_DEVICE_COMPILE__
    const float len = __builtin_amdgcn_sqrtf(s2);
#else
    const float len = __builtin_sqrtf(s2);
#endif
    const float lb = (len - rf) - (len + __builtin_fabsf(rf) + 1.0f) * 4e-6f;
    return key != 0xFFFFFFFFu && s2 < __builtin_inff() ? lb : __builtin_inff();
}
// That bound on its way from section B to section M, in the upper half of a word (NormalAux::k1, rm_render_v2.hip).  The upper
// half of a binary32 number is the number with its mantissa cut to seven bits: the cut moves a value towards zero by less than
// 2^-7 of its magnitude, so the value is lowered by 2^-6 of its magnitude first and what is unpacked never exceeds what was
// packed, and is at least 0.97 of a positive one.  +inf stays +inf, a NaN a NaN; only a negative denormal can come out raised,
// by less than 2^-126.
inline __host__ __device__ uint32_t rm_runner_up_pack_bound(float lb3) {
    const float mag = __builtin_fabsf(lb3);
    const float low = lb3 - (mag < 3.0e38f ? mag : 3.0e38f) * 0.015625f;
    return __builtin_bit_cast(uint32_t, low) & 0xFFFF0000u;
}
inline __host__ __device__ float rm_runner_up_unpack_bound(uint32_t word) { return __builtin_bit_cast(float, word & 0xFFFF0000u); }

// rm_compare_frames_device (rm_frame_ops.hip, compare_kernel).  The maps are rm_compare_map's values.
enum { RM_CMP_NONE = -1, RM_CMP_SDF = 0, RM_CMP_ITERS = 1, RM_CMP_DEPTH = 2, RM_CMP_NORMAL = 3, RM_CMP_SURFACE = 4 };
struct RmCompareStats {  // rm_compare_stats: sums = sum_sdf_a .. a_cheaper in the order of the header
    unsigned long long pixels;
    unsigned long long sums[14];
    unsigned int max_abs_depth, max_abs_normal;
};
struct RmComparePartial {  // what one workgroup of a frame contributes: the 14 sums, then the two maxima
    unsigned long long v[16];
};
struct RmCompareArgs {
    const uint8_t *depth_a, *depth_b, *normal_a, *normal_b;  // a pair is present or absent on both sides
    const uint16_t *sdf_a, *sdf_b, *iters_a, *iters_b;
    uint8_t *rgba;               // null exactly when the map is RM_CMP_NONE
    RmCompareStats *stats;       // one record per frame, or null
    RmComparePartial *partials;  // [n_frames][blocks_per_frame], and ...
    unsigned int *counters;      // ... the frame's ticket counter at [frame * blocks_per_frame], zero before and after the launch;
                                 // both unused (may be null) with one workgroup per frame or without stats
    long long npx;               // pixels of a frame
    unsigned int gain;
};

// rm_counter_hist_device / rm_shade_ranged_device (rm_frame_ops.hip, hist_kernel and shade_ranged_kernel).
constexpr int RM_HIST_NBINS = 256;
struct RmCounterHist {  // rm_counter_hist
    unsigned long long pixels, sum;
    unsigned int min, max, range_lo, range_hi, shift, reserved;
    unsigned int bins[RM_HIST_NBINS];
};
struct RmFrameHist {  // rm_frame_hist
    RmCounterHist sdf, iters;
};
struct RmHistScratch {  // what the workgroups of one frame add into (index 0 sdf, 1 iters); all zero before and after the launch
    unsigned int bins[2][RM_HIST_NBINS];
    unsigned long long sum[2];
    unsigned int max[2], inv_min[2];  // inv_min: the maximum of ~v, so that zero is neutral
    unsigned int ticket, pad[3];
};
struct RmHistArgs {
    const uint16_t *sdf, *iters;  // either may be null
    const uint8_t *normal;        // read by hist_kernel<true> only
    RmFrameHist *hist;            // one per frame
    RmHistScratch *scratch;       // one per frame; unused (may be null) with one workgroup per frame
    long long npx;                // pixels of a frame
    unsigned int shift, lo_permille, hi_permille;
    unsigned int want_surface;    // hist_kernel<true>: 1 counts surface pixels, 0 background pixels
};
struct RmShadeRangedArgs {
    const uint16_t *values;
    const RmFrameHist *hist;  // null: lo and hi below for every frame
    uint8_t *rgba;
    long long npx;
    unsigned int counter, lo, hi;  // counter: 0 takes hist[k].sdf, 1 hist[k].iters
};
// rm_shade_lit_device (rm_frame_ops.hip, shade_lit_kernel): frame k at element k * npx of every buffer (x3 normal, x4 rgba)
struct RmShadeLitArgs {
    const uint8_t *depth, *normal;
    const float *lit, *ao;
    uint8_t *rgba;
    long long npx;
    double light[3];  // PhongModel's binary32 light direction, widened (exact)
};
// The ray queries (rm_kernels.hip).  RmRays: the rays of one launch, handed to the launchers beside the family's block.  The
// kernels take their arguments where they took them before the launchers were unified: cast and pick loose, light and walk
// their block with the rays in it.  (A block that opens with RmRays, for all four kernels, cost the BVH sphere kernels SGPR
// spills and about 1 % on the C3 rays: profiles/NOTES.md.)  Every output may be null.
struct RmRays {
    const float *origins, *dirs;  // f32[3n]
    long long n;
};
// rm_ray_march (cast_kernel) and rm_ray_pick (pick_kernel, which alone reads slot_obj and writes object)
struct RmQueryArgs {
    int32_t want_normal, pad;
    const int32_t *slot_obj;  // device sphere slot -> object index (sphere scenes stored in BVH leaf order), null when the two agree
    double *t;
    uint32_t *iters, *sdf;
    float *normal;            // written whether or not want_normal is set (zeros without)
    int32_t *object;          // i32[n], -1 = none
};
// rm_ray_light (light_kernel): the outputs and the rm_light of one launch
struct RmLightArgs {
    const float *origins, *dirs;  // set by the launcher: its RmRays
    double *t;                    // the primary ray's outputs: what cast_kernel writes with want_normal
    uint32_t *iters, *sdf;
    float *normal;
    float *lit, *ao;              // f32[n]
    uint32_t *iters2, *sdf2;      // the shadow ray's iterations; its SDF calls plus those of the occlusion samples
    long long n;                  // set by the launcher
    double bias, ao_step, ao_strength;
    float light[3];               // towards the light, as given
    int ao_samples;
};
// rm_ray_walk (walk_kernel): rm_step and rm_walk as the kernel stores them, and the outputs of one launch.  steps: cap slots
// per ray, null for summaries only (the same for every lane); walks may be null when steps is not.
struct RmWalkStep {  // rm_step (24 bytes)
    double t, value;
    uint32_t count;
    int32_t kind;
};
struct RmWalkSummary {  // rm_walk (48 bytes)
    double t, min_dist, t_min, skipped;
    uint32_t evals, skips, sdf_calls;
    int32_t end;
};
struct RmWalkArgs {
    const float *origins, *dirs;  // set by the launcher: its RmRays
    RmWalkSummary *walks;
    RmWalkStep *steps;
    long long n;                  // set by the launcher
    int cap, pad;
};
// The lattice of the field, sharp-vertex and mesh launches: rm_lattice's binary32 vectors, widened (exact).  It is the first
// member of every argument block that names a lattice, so the vectors sit where they sat when each block spelled them out (the
// static_asserts ahead of the launchers' declarations pin the layouts: the kernels take the blocks by value).
struct RmLattice {
    double origin[3], du[3], dv[3], dw[3];
};
// The point rule of include/rm_raymarch.h, the contract of every lattice entry: component c of the point with index (fi, fj, fk)
// -- whole numbers for a lattice point, fractional ones for a mesh vertex or an edge crossing -- in binary64, left to right, one
// operation at a time (-ffp-contract=off).  This is the rule's only text on the device: field values, tiles, mesh vertices and
// sharp vertices agree bit for bit because all of them call it.  A point is its three components, each rounded once to binary32
// (rm_kernels.hip, lattice_point); the sharp vertices also take a component before its rounding.  (The library's own
// kernels only: a scene kernel compiled at run time samples no lattice.)
#if defined(__HIP__) && !defined(RM_RTC)
__device__ __forceinline__ double rm_lattice_component(const RmLattice &l, int c, double fi, double fj, double fk) {
    return ((l.origin[c] + fi * l.du[c]) + fj * l.dv[c]) + fk * l.dw[c];
}
#endif
// rm_scene_field (rm_kernels.hip, field_kernel): the lattice, the linear range [first, first + n) of one call and the outputs,
// indexed from `first`, each of which may be null
struct RmFieldArgs {
    RmLattice lat;
    double *dist;
    float *dist32;
    uint32_t *count;
    long long first, n;
    long long block_first;  // set by the launcher: the first of the range's workgroups this launch runs
    unsigned int nu, nv;
};
// rm_scene_points (rm_kernels.hip, point_kernel): n points, the query and the outputs, each of which may be null; position may
// be points (a lane reads its point before it writes)
struct RmPointArgs {
    const float *points;      // f32[3n]
    float *position;          // f32[3n]
    double *dist;
    float *normal;            // f32[3n]: zeros without want_normal
    int32_t *object;          // i32[n], -1 = none: computed only when asked for
    int32_t *steps;
    uint32_t *count;
    const int32_t *slot_obj;  // as RmQueryArgs::slot_obj
    long long n;
    double iso, snap_tol;
    int32_t snap_steps, want_normal;
};
// rm_scene_sharpen (rm_kernels.hip, sharp_kernel): n vertices named by the keys of their cells, RM_SHARP_CELLS consecutive ones
// per workgroup of 256 lanes (include/rm_raymarch.h, "sharp meshes", has the rule)
#define RM_SHARP_CELLS 64
#define RM_SHARP_CROSSINGS (12 * RM_SHARP_CELLS)  // what the cells of a workgroup can hold at most
struct RmSharpArgs {
    RmLattice lat;
    double iso, rank_tol;
    double limit;             // reach * rho, formed by the host in the rule's order
    const long long *cells;   // i64[n]
    float *position;          // f32[3n]
    int32_t *feature;         // i32[n], may be null
    uint32_t *count;          // u32[n], may be null
    long long n;
    unsigned int nu, nv, nw;
    int32_t refine;
};
// rm_shade_field_device (rm_frame_ops.hip, shade_field_kernel): n values (f64 distances or u32 counts) -> n pixels
struct RmShadeFieldArgs {
    const void *values;
    uint8_t *rgba;
    long long n;
    double range, band, line;
    unsigned int lo, hi;
    int map, pad;  // 0 distance, 1 count
};
// rm_mesh_field_device / rm_scene_mesh (rm_mesh.hip): surface nets over the n = nu * nv * nw values of a lattice.
#define RM_MESH_BLOCK 256       // points per workgroup of the three per-point kernels
#define RM_MESH_SCAN_STEP 1024  // block totals mesh_scan_kernel takes per step of its loop
struct RmMeshInfo {  // rm_mesh_info (32 bytes)
    long long n_vertices, n_quads, n_holes, reserved;
};
struct RmMeshArgs {
    RmLattice lat;
    const void *values;  // n binary64 values, or binary32 ones with f32
    double iso;
    float *vertices;     // cap_vertices x 3
    uint32_t *quads;     // cap_quads x 4
    RmMeshInfo *info;
    uint32_t *map;       // n words: the vertex of the cell whose low corner the point is, or 0xFFFFFFFF
    uint32_t *totals;    // 3 x n_blocks words: active cells, quads and holes per workgroup; the first two become offsets
    long long n, cap_vertices, cap_quads;
    unsigned int nu, nv, nw, n_blocks;  // n_blocks = ceil(n / RM_MESH_BLOCK)
    int f32, pad;
};
// The sparse mesher (rm_scene_blocks_device, rm_scene_tiles_device, rm_mesh_tiles_device): blocks of RM_SPARSE_BLOCK^3 cells,
// each with a tile of (RM_SPARSE_BLOCK + 1)^3 lattice points.  include/rm_raymarch.h ("sparse meshes") has the rule.
#define RM_SPARSE_BLOCK 8
#define RM_SPARSE_TILE 729          // 9 * 9 * 9 values of a tile, a fastest
#define RM_SPARSE_CELLS 512         // cells of a block, local index (z * 8 + y) * 8 + x
#define RM_SPARSE_MAX_BLOCKS (1 << 24)
#define RM_SPARSE_MAX_KEPT (1 << 21)  // what rm_mesh_tiles_device takes: 2^30 cells, so vertex and quad numbers fit 32 bits
struct RmSparseInfo {  // rm_sparse_info (32 bytes)
    long long n_blocks, n_kept, reserved[2];
};
// The coarse pass (rm_kernels.hip blocks_kernel, then rm_mesh_sparse.hip): one lane per block.  blocks_kernel writes the keep
// flag (0 kept, -1 dropped) into slot and the kept blocks of each workgroup of 256 into totals; the scan turns the totals into
// offsets and writes info; the scatter turns the flags into ranks and writes list.
struct RmBlocksArgs {
    RmLattice lat;
    double iso, bound;
    int32_t *slot, *list;
    double *dist;       // may be null
    RmSparseInfo *info;
    uint32_t *totals;   // ceil(n_blocks / 256) words
    unsigned int nu, nv, nw, nbu, nbv, nbw;
    unsigned int n_blocks, n_groups;
};
// rm_scene_tiles_device (rm_kernels.hip tiles_kernel): one workgroup per kept block
struct RmTilesArgs {
    RmLattice lat;
    const int32_t *list;
    double *tiles;      // n_kept x RM_SPARSE_TILE
    unsigned int nu, nv, nw, nbu, nbv, n_kept;
    // read by the exact launch only: what a tile point is away from the tile's centre point at most, per axis and in all
    // (4 (|du| + |dv| + |dw|), the coarse pass's R, and its slack for the roundings)
    double half[3], radius;
};
// rm_scene_tiles_update_device (rm_kernels.hip tiles_update_kernel): what the update reads beside the tile launch's RmTilesArgs
struct RmBall {  // rm_ball (24 bytes)
    float center[3];
    int32_t reserved;
    double radius;
};
struct RmTilesUpdateInfo {  // rm_tiles_update_info (32 bytes)
    long long n_kept, n_reused, n_evaluated, reserved;
};
#define RM_UPDATE_MAX_BALLS (1 << 16)
struct RmTilesUpdateArgs {
    const int32_t *prev_slot;   // n_blocks: the previous scene's slot map
    const double *prev_tiles;   // n_prev_kept x RM_SPARSE_TILE
    const RmBall *balls;
    int32_t *reused;            // n_kept flags (1: the tile was copied), or null
    unsigned int n_blocks, n_prev_kept;
    int n_balls, pad;
};
// Option `exact`: the value of RmRenderParams::accel in a point, field or tile launch that evaluates the exact field
// (rm_kernels.hip, exact_distance).  Such a launch names the tree to walk in bvh / bvh_prims / bvh_nodes -- the scene's BVH or
// its exact tree -- and bvh_nodes = 0 where every object is evaluated.
#define RM_ACCEL_EXACT 3
// rm_mesh_tiles_device (rm_mesh_sparse.hip): one workgroup per kept block, the fields vertex_position reads named as in RmMeshArgs
struct RmSparseMeshArgs {
    RmLattice lat;
    double iso;
    const int32_t *slot, *list;
    const double *tiles;
    float *vertices;
    uint32_t *quads;
    long long *cells, *edges;  // the dense mesher's sort keys per vertex and per quad; each may be null
    RmMeshInfo *info;
    uint32_t *map;       // n_kept x RM_SPARSE_CELLS words: the vertex of the cell, or 0xFFFFFFFF
    uint32_t *totals;    // 3 x n_kept words, as RmMeshArgs::totals with one workgroup per kept block
    long long cap_vertices, cap_quads;
    unsigned int nu, nv, nw, nbu, nbv, nbw, n_kept, pad;
};
// rm_measure_field_device / rm_measure_tiles_device (rm_measure.hip): integer sums over the inside points of a lattice.
#define RM_MEASURE_SUMS 15
struct RmMeasure {  // rm_measure (176 bytes)
    long long n_points, n_inside, n_nonfinite, sum1[3], sum2[6], crossings[3];
    int lo[3], hi[3];
    long long n_blocks, n_kept, n_blocks_inside, reserved;
};
// what one workgroup found: n_inside, n_nonfinite, sum1, sum2, crossings, n_blocks_inside in that order, and its box
struct RmMeasurePartial {  // 144 bytes
    long long sum[RM_MEASURE_SUMS];
    int lo[3], hi[3];
};
struct RmMeasureFieldArgs {
    const void *values;  // n binary64 values, or binary32 ones with f32
    double iso;
    RmMeasurePartial *partials;  // one per workgroup of the launch
    RmMeasure *out;
    long long n;
    unsigned int nu, nv, nw;
    int f32;
};
struct RmMeasureTilesArgs {
    double iso;
    const int32_t *slot, *list;
    const double *dist, *tiles;
    RmMeasurePartial *partials;  // n_kept, then one per workgroup of measure_blocks_kernel
    RmMeasure *out;
    long long n;
    unsigned int nu, nv, nw, nbu, nbv, nbw, n_blocks, n_kept;
};
// rm_label_field_device / rm_measure_labels_device (rm_parts.hip): the connected parts of the points on one side of iso.
#define RM_PARTS_MAX_RECORDS (1 << 20)
struct RmPartsInfo {  // rm_parts_info (32 bytes)
    long long n_points, n_set, n_parts, gave_up;
};
struct RmPartsArgs {
    const void *values;  // n binary64 values, or binary32 ones with f32
    double iso;
    int32_t *labels;     // n words: the union-find's parent array, then the part numbers
    uint32_t *map;       // n words: a root's part number
    uint32_t *totals;    // 2 x n_blocks words: roots (they become offsets) and points of the set per workgroup
    RmPartsInfo *info;   // zeroed ahead of the launch
    long long n;
    unsigned int nu, nv, nw, n_blocks;  // n_blocks = ceil(n / RM_MESH_BLOCK)
    int f32, outside;
};
struct RmPartsMeasureArgs {
    const int32_t *labels;
    RmMeasure *records;  // n_records of them
    long long n;
    unsigned int nu, nv, nw, n_records;
};
// rm_edt_field_device (rm_edt.hip): the squared index distance of every point on one side of iso to the nearest point on the other.
#define RM_EDT_PARTIAL_BYTES (16 * 1024)  // edt_reduce_kernel's partials: 1024 workgroups at most, 16 bytes each
struct RmEdtInfo {  // rm_edt_info (32 bytes)
    long long n_points, n_set, max_d2, argmax;
};
struct RmEdtArgs {
    const void *values;         // n binary64 values, or binary32 ones with f32
    double iso;
    int32_t *d2;                // n words: the result, every pass in place
    unsigned long long *stack;  // n entries: a line's envelope, entry q where the line's q-th point is in the volume
    void *partials;             // RM_EDT_PARTIAL_BYTES
    RmEdtInfo *info;
    long long n;
    unsigned int nu, nv, nw;
    int f32, outside;
};
// The device scene builder (rm_scene_build.hip): the pair loops of rm_scene_host.h's PairLoops.
// A candidate grid: cell (x, y, z) is the box org + (x - 0.03) * w .. org + (x + 1.03) * w per axis (the host's cell with
// its 3 % slack; org and w are the host's own binary64 values), its spheres the n entries from `first` on of the launch's
// id table -- or, without one, of its sphere table.
struct RmCandGrid {
    double org[3], w[3];
    int32_t dim[3];
    int32_t first, n, pad;
};
#define RM_CAND_NO_LIST 0xFFFFFFFFu  // counts / offsets: the cell keeps no list
// One launch of the candidate rule over n_grids grids of cells_per_grid cells each (= dim[0] * dim[1] * dim[2] of every
// grid), cells numbered grid after grid, x fastest.  Pass 1 (rm_launch_cand_count) writes counts and u; the caller turns
// the counts into offsets; pass 2 (rm_launch_cand_fill) reads offsets and u and writes the lists.
struct RmCandArgs {
    const RmCandGrid *grids;
    const double *spheres;  // per sphere cx, cy, cz (the binary32 centre, widened) and the radius
    const int32_t *ids;     // sphere ids the grids' ranges index, or null
    uint32_t *counts;       // pass 1, per cell: spheres with lb <= U + 1e-6, or RM_CAND_NO_LIST (use_root: the cell lies inside the root box)
    double *u;              // per cell: U = min(u0, min_j ub_j)
    const uint32_t *offsets;  // pass 2, per cell: where its list starts, or RM_CAND_NO_LIST
    long long n_cells;      // n_grids * cells_per_grid
    unsigned long long list_len;  // entries the list buffer of pass 2 holds
    double u0;
    double root_lo[3], root_hi[3];
    int32_t n_grids, cells_per_grid, n_spheres, n_ids, use_root, pad;
};
// OctBuilder::nearest_prim_box for n_nodes node boxes (lo[3], hi[3] per node) against n_prims primitive boxes
struct RmEmptyDistArgs {
    const float *boxes, *prim_lo, *prim_hi;
    double *out;  // per node: max(0, min_i box_gap(node, prim i)), 0 without a primitive
    int32_t n_nodes, n_prims;
};

#ifndef __HIPCC_RTC__  // (host side: the launchers)
// The blocks that open with the lattice are kernel arguments by value, filled by rm_api.cpp and read by the kernels: their layout
// is an ABI between the two.  The sizes, and where the first member behind the vectors starts, as they were when every block
// spelled the four vectors out.
static_assert(sizeof(RmLattice) == 96, "the lattice's four vectors");
static_assert(sizeof(RmFieldArgs) == 152 && offsetof(RmFieldArgs, dist) == 96, "RmFieldArgs layout");
static_assert(sizeof(RmSharpArgs) == 176 && offsetof(RmSharpArgs, iso) == 96, "RmSharpArgs layout");
static_assert(sizeof(RmMeshArgs) == 200 && offsetof(RmMeshArgs, values) == 96, "RmMeshArgs layout");
static_assert(sizeof(RmBlocksArgs) == 184 && offsetof(RmBlocksArgs, iso) == 96, "RmBlocksArgs layout");
static_assert(sizeof(RmTilesArgs) == 168 && offsetof(RmTilesArgs, list) == 96, "RmTilesArgs layout");
static_assert(sizeof(RmSparseMeshArgs) == 232 && offsetof(RmSparseMeshArgs, iso) == 96, "RmSparseMeshArgs layout");

// rm_scene_build.hip.  elem_bytes: 2 (uint16_t lists: the two grids) or 1 (uint8_t: octree sub-cells)
hipError_t rm_launch_cand_count(const RmCandArgs &a, hipStream_t stream);
hipError_t rm_launch_cand_fill(const RmCandArgs &a, void *list, int elem_bytes, hipStream_t stream);
hipError_t rm_launch_empty_dist(const RmEmptyDistArgs &a, hipStream_t stream);
// rmh::js_hypot3 of n binary64 triples as the device builder evaluates it (rm_selftest_hypot64)
hipError_t rm_launch_hypot64(const double *xyz, int64_t n, double *out, hipStream_t stream);

// Renders rows [y_start, y_end) (runRaymarcher + optional fused shade).  *kernel_name (optional) receives the
// instantiation that was launched (static string); v2_shape (optional) what a launch of the v2 wave loop was launched with:
// workgroups, threads per workgroup, dynamic LDS bytes, whether it took the step-box table and whether the leaf rectangles:
// five words (left alone by every other launch).
hipError_t rm_launch_render(const RmRenderParams &p, hipStream_t stream, const char **kernel_name, uint32_t *v2_shape = nullptr);
hipError_t rm_launch_render_sqrt(const RmRenderParams &p, hipStream_t stream, const char **kernel_name, uint32_t *v2_shape = nullptr);

// Asked by rm_launch_render_v2 for every launch that carries a context (RmRenderParams::rtc_ctx): the hipFunction_t of the
// wave loop compiled for this launch's configuration (rm_v2_fields.h), or null -- the library's own instantiation runs.
// Implemented in rm_api.cpp (it counts how often a configuration comes back and owns the compile policy).
const void *rm_rtc_v2_hook(const RmRenderParams &p, int accel, bool lds, bool ur, bool rel, bool length_sqrt);

// v2 kernel (rm_render_v2.hip); called by rm_launch_render when p.variant == 2
hipError_t rm_launch_render_v2(const RmRenderParams &p, hipStream_t stream, const char **kernel_name, uint32_t *shape = nullptr);
hipError_t rm_launch_render_v2_sqrt(const RmRenderParams &p, hipStream_t stream, const char **kernel_name, uint32_t *shape = nullptr);

// The second stage of the launch fill (option `overlap_fill`): a launch whose floor is `floor_per_cu` workgroups
// per CU brings `candidate` instead when every one of its waves still gets RM_V2_OVERLAP_ITEMS_PER_WAVE of the frame's `items`
// (tiles_x * tiles_y work items) -- what a workgroup's start, ~20 KB of tables staged into LDS, has to be paid with.  The
// threshold is measured (profiles/NOTES.md, round 6).  One definition for the launcher and rm_debug_overlap_fill.
#define RM_V2_OVERLAP_ITEMS_PER_WAVE 3
inline int rm_v2_overlap_per_cu(int floor_per_cu, int candidate, long long items, int cus) {
    if (candidate <= floor_per_cu || cus <= 0) return floor_per_cu;
    const long long needed = (items + 3) / 4, resident = static_cast<long long>(cus) * candidate;
    const long long waves = 4 * (needed < resident ? needed : resident);
    return items >= RM_V2_OVERLAP_ITEMS_PER_WAVE * waves ? candidate : floor_per_cu;
}

// Whether rm_leaf_rect's premise holds for a camera: finite, and the columns of `rot` orthonormal within 1e-6 (every pairwise
// dot product against the identity, in binary64; a rotation rounded to binary32 is within 2e-7).  One definition for
// fill_params and the debug entries.
inline bool rm_rect_cull_camera_ok(const float rot[9], const float origin[3]) {
    for (int k = 0; k < 3; ++k)
        if (!(origin[k] - origin[k] == 0.f)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += static_cast<double>(rot[3 * i + k]) * static_cast<double>(rot[3 * j + k]);
            const double err = d - (i == j ? 1.0 : 0.0);
            if (!(err >= -1e-6 && err <= 1e-6)) return false;
        }
    return true;
}

// What a launch of the v2 wave loop keeps in LDS, decided from its parameters alone (no device): the scene's tables (lds), the
// origin-relative node boxes (rel), list_cap entries of hit list per ray, and the step-box table of section M (step_box: asked
// for through RmRenderParams::step_box and granted; refused: asked for, but it would have cost the scene's staging, the
// relative boxes or a workgroup per CU).  tier: which LDS budget the launch reaches (0: the first; rm_render_v2.hip).
// cell_on: the launch reads its candidates from the scene's cell table and does not stage the point-query grid (asked for
// through RmRenderParams::cell_on; granted when the step-box table is taken, the scene stays staged, the same budget is
// reached and the hit lists are no shorter than without it); cell_refused: asked for and not granted.
struct RmV2Plan {
    bool lds, rel;
    int list_cap, step_box, tier, refused, cell_on, cell_refused;
    int runner_up;  // section M bounds the runner-up by its own distance (asked for through RmRenderParams::runner_up; granted to a one-radius launch that took the cell table)
    int per_cu;  // workgroups of the launch that a CU's LDS holds (at most RM_V2_WAVES: the registers')
    size_t scene_bytes, list_bytes;
};
RmV2Plan rm_v2_plan(const RmRenderParams &p);

// rm_debug_wave_distance: Scene.getDistance through the wave loop's bvh_distance_wave, one point per lane (BVH sphere scenes)
hipError_t rm_launch_wave_distance(const RmRenderParams &p, const float *points, int64_t n, double *dist, uint32_t *count, hipStream_t stream);
hipError_t rm_launch_wave_distance_sqrt(const RmRenderParams &p, const float *points, int64_t n, double *dist, uint32_t *count, hipStream_t stream);

// the octree's node boxes relative to one camera position, for render_kernel_oct (rm_kernels.hip)
hipError_t rm_launch_oct_frame_table(const RmOctNode *nodes, int n, const double origin[3], RmOctFrameNode *out, hipStream_t stream);

// ShadingModel.shade over n = width * height pixels.
hipError_t rm_launch_shade(int shader, int64_t n, const uint8_t *depth, const uint8_t *normal,
                           const uint16_t *sdf, const uint16_t *iters, uint8_t *rgba,
                           const float light[3], hipStream_t stream);

// sums 0, max 0, min UINT_MAX
hipError_t rm_launch_reduce_init(RmDiagDevice *acc, hipStream_t stream);

// diagnostics reduction into *acc (must be initialised: sums 0, max 0, min UINT_MAX)
hipError_t rm_launch_reduce(const uint16_t *sdf, const uint16_t *iters, int64_t n, RmDiagDevice *acc,
                            hipStream_t stream);

// Scene.getDistance for a batch of points
hipError_t rm_launch_distance(const RmRenderParams &p, const float *points, int64_t n, double *dist,
                              uint32_t *count, hipStream_t stream);
hipError_t rm_launch_distance_sqrt(const RmRenderParams &p, const float *points, int64_t n, double *dist,
                                   uint32_t *count, hipStream_t stream);

// Ray queries: r.n caller-supplied rays through the march of a one-ray-per-lane render launch, one launch of 256-thread
// workgroups with that launch's LDS.  The four launchers share one prologue (rm_kernels.hip, ray_launch) and differ in the kernel
// they name and in how they hand it its arguments.  *kernel_name (optional) receives the instantiation that was launched (static string).
// rm_ray_march (cast_kernel) and rm_ray_pick (pick_kernel): Raymarcher.rayMarch (+ getNormal when a.want_normal); pick_kernel
// also writes the object each ray hit, cast_kernel reads neither a.slot_obj nor a.object.
hipError_t rm_launch_cast(const RmRenderParams &p, const RmRays &r, const RmQueryArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_cast_sqrt(const RmRenderParams &p, const RmRays &r, const RmQueryArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_pick(const RmRenderParams &p, const RmRays &r, const RmQueryArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_pick_sqrt(const RmRenderParams &p, const RmRays &r, const RmQueryArgs &a, hipStream_t stream, const char **kernel_name);
// rm_ray_light (light_kernel): the march with its normal, then at hits one shadow ray towards a.light through the same marcher
// and a.ao_samples Scene.getDistance samples along the normal (include/rm_raymarch.h has the rule).
hipError_t rm_launch_light(const RmRenderParams &p, const RmRays &r, const RmLightArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_light_sqrt(const RmRenderParams &p, const RmRays &r, const RmLightArgs &a, hipStream_t stream, const char **kernel_name);
// rm_ray_walk (walk_kernel): the march without a normal, with a recorder that keeps the walk's summary and stores its first
// a.cap step records (include/rm_raymarch.h has the rule).
hipError_t rm_launch_walk(const RmRenderParams &p, const RmRays &r, const RmWalkArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_walk_sqrt(const RmRenderParams &p, const RmRays &r, const RmWalkArgs &a, hipStream_t stream, const char **kernel_name);

// The queries that sample the scene at points and have no ray: field, points, sharp vertices, and the sparse mesher's blocks and
// tiles below.  The five launchers share one prologue (rm_kernels.hip, scene_launch): 256-thread workgroups, the dynamic LDS of
// rm_launch_distance (no hit-leaf lists) and the parameter block without a run-time specialised kernel or diagnostics --
// ahead-of-time kernels only.  Each is left with its guard, its grid and the line that names its kernel.
// Field query (rm_scene_field): Scene.getDistance at the lattice points of a.first .. a.first + a.n, formed on the device
// (include/rm_raymarch.h has the rule; rm_lattice_component above is its text).  field_kernel.
hipError_t rm_launch_field(const RmRenderParams &p, const RmFieldArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_field_sqrt(const RmRenderParams &p, const RmFieldArgs &a, hipStream_t stream, const char **kernel_name);

// Point query (rm_scene_points): distance, gradient, object and up to a.snap_steps projection steps for a.n caller-supplied
// points, one per lane (include/rm_raymarch.h has the rule).  point_kernel; 0 <= a.n <= INT32_MAX.
hipError_t rm_launch_points(const RmRenderParams &p, const RmPointArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_points_sqrt(const RmRenderParams &p, const RmPointArgs &a, hipStream_t stream, const char **kernel_name);

// Sharp vertices (rm_scene_sharpen): sharp_kernel, one workgroup per RM_SHARP_CELLS vertices, the prologue's LDS beside its own
// static arrays; 0 <= a.n <= INT32_MAX.
hipError_t rm_launch_sharp(const RmRenderParams &p, const RmSharpArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_sharp_sqrt(const RmRenderParams &p, const RmSharpArgs &a, hipStream_t stream, const char **kernel_name);

// Surface nets (rm_mesh.hip): count, scan and -- with a capacity above 0 -- the two emit kernels, back to back on `stream`.
// a.map and a.totals are the caller's scratch; 1 <= a.n <= 2^30.
hipError_t rm_launch_mesh(const RmMeshArgs &a, hipStream_t stream, const char **kernel_name);
// rm_mesh_cells_device: the same count and scan, then the key of every active cell at its vertex number into a.cells
// (a.vertices, a.quads and a.map are not read; a.cap_quads is 0).
hipError_t rm_launch_mesh_cells(const RmMeshArgs &a, long long *cells, hipStream_t stream, const char **kernel_name);

// The sparse mesher.  rm_launch_blocks (rm_kernels.hip): blocks_kernel<GEN, WALK> -- the exact distance at every block centre,
// by the pruned walk of the BVH where the scene has one and is no expression program, else over all objects -- and, through
// rm_launch_blocks_compact (rm_mesh_sparse.hip), the scan and the scatter.  rm_launch_tiles (rm_kernels.hip): tiles_kernel<ACCEL,
// GEN>.  rm_launch_mesh_tiles (rm_mesh_sparse.hip): count, scan and -- with a capacity above 0 -- the two emit kernels.
// 1 <= n_blocks <= RM_SPARSE_MAX_BLOCKS; 1 <= n_kept (RM_SPARSE_MAX_KEPT for the mesher).
hipError_t rm_launch_blocks(const RmRenderParams &p, const RmBlocksArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_blocks_sqrt(const RmRenderParams &p, const RmBlocksArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_blocks_compact(const RmBlocksArgs &a, hipStream_t stream);
hipError_t rm_launch_tiles(const RmRenderParams &p, const RmTilesArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_tiles_sqrt(const RmRenderParams &p, const RmTilesArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_mesh_tiles(const RmSparseMeshArgs &a, hipStream_t stream, const char **kernel_name);
// rm_launch_tiles_update (rm_kernels.hip): tiles_update_kernel<GEN> over a.n_kept blocks, sphere and primitive records only
// (p.general < 2, p.accel == RM_ACCEL_EXACT).  rm_launch_tiles_update_totals (rm_mesh_sparse.hip): the n_kept flags -> info,
// one workgroup, plain sums.
hipError_t rm_launch_tiles_update(const RmRenderParams &p, const RmTilesArgs &a, const RmTilesUpdateArgs &u, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_tiles_update_sqrt(const RmRenderParams &p, const RmTilesArgs &a, const RmTilesUpdateArgs &u, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_tiles_update_totals(const int32_t *reused, unsigned int n_kept, RmTilesUpdateInfo *info, hipStream_t stream);
// The measures (rm_measure.hip).  rm_launch_measure_field: measure_field_kernel<T> over n_groups workgroups, then
// measure_final_kernel; 0 <= a.n <= 2^30, and n_groups = rm_measure_field_groups(...) partials (0 without a point: the final
// kernel alone writes the empty record).  rm_launch_measure_tiles: measure_tiles_kernel over a.n_kept workgroups (none: not
// launched), measure_blocks_kernel over n_groups = rm_measure_block_groups(...) workgroups, measure_final_kernel;
// a.partials holds a.n_kept + n_groups records.  The grids are persistent: num_cus bounds them.
unsigned int rm_measure_field_groups(long long n, unsigned int nv, unsigned int nw, int num_cus);
unsigned int rm_measure_block_groups(unsigned int n_blocks, int num_cus);
hipError_t rm_launch_measure_field(const RmMeasureFieldArgs &a, unsigned int n_groups, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_measure_tiles(const RmMeasureTilesArgs &a, unsigned int n_groups, hipStream_t stream, const char **kernel_name);
// The parts (rm_parts.hip).  rm_launch_label_field: parts_init_kernel<T>, parts_merge_kernel, parts_flatten_kernel, parts_scan_kernel,
// parts_number_kernel and parts_relabel_kernel over a.n_blocks workgroups each (the scan: one); 0 < a.n <= 2^30 and *a.info zeroed
// on the stream beforehand.  rm_launch_measure_labels: parts_records_kernel over the a.n_records records (none: not launched),
// then parts_measure_kernel over a persistent grid that num_cus bounds (no point: not launched); 0 <= a.n <= 2^30.
hipError_t rm_launch_label_field(const RmPartsArgs &a, hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_measure_labels(const RmPartsMeasureArgs &a, int num_cus, hipStream_t stream, const char **kernel_name);
// The distance transform (rm_edt.hip): edt_rows_kernel<T> over ceil(a.n / RM_MESH_BLOCK) workgroups, edt_axis_kernel along j and
// along k over a lane per line (an axis of one point: not launched), edt_reduce_kernel and edt_info_kernel; 0 < a.n <= 2^30 and
// (nu-1)^2 + (nv-1)^2 + (nw-1)^2 <= INT32_MAX - 1.  *kernel_name: edt_axis_kernel, or edt_rows_kernel where no axis pass ran.
hipError_t rm_launch_edt_field(const RmEdtArgs &a, hipStream_t stream, const char **kernel_name);

// rm_render_frames_device: frame k of n_views is rows [y_start, y_end) of p with views[k] (device table) for p's rot, origin,
// origin_d and time, its pixels at element k * width * local_rows of every buffer p names (x3 normal, x4 rgba), its diagnostics
// (acc non-null) accumulated in blocks[k] (zero before and after the launch) and written to acc[k].  One launch of
// frames_kernel; frames without a pixel: the neutral elements to acc[0 .. n_views).
hipError_t rm_launch_frames(const RmRenderParams &p, const RmFrameView *views, int32_t n_views, RmFrameDiagBlock *blocks, RmDiagDevice *acc,
                            hipStream_t stream, const char **kernel_name);
hipError_t rm_launch_frames_sqrt(const RmRenderParams &p, const RmFrameView *views, int32_t n_views, RmFrameDiagBlock *blocks, RmDiagDevice *acc,
                                 hipStream_t stream, const char **kernel_name);

// v2: builds the longest-first item order of the next launch from the previous launch's recorded costs (rm_render_v2.hip)
hipError_t rm_launch_lpt_sort(const uint8_t *cost_prev, uint16_t *perm, int stride, int tiles_x, int tiles_y, hipStream_t stream);

// Rank 0 of a sharded frame (rm_frame_ops.hip): copies every stripe of a gathered [world x rank_stride] buffer to its
// place in the row-major frame and combines the ranks' partial diagnostics accumulators.
hipError_t rm_launch_assemble(const unsigned char *gathered, int64_t rank_stride, int64_t section_offset, int32_t row_bytes,
                              int32_t height, int32_t stripe_rows, const int32_t *stripe_src, int32_t n_stripes,
                              unsigned char *frame, int64_t acc_offset, int32_t world, RmDiagDevice *acc, hipStream_t stream);

// rm_compare_frames_device: ONE launch of compare_kernel<map, stats> over n_frames frames of a.npx pixels, blocks_per_frame
// workgroups each (rm_compare_blocks_per_frame: what the caller sizes a.partials and a.counters by).  Launches nothing when
// there is no pixel, no frame, or neither an image nor statistics to write.
int32_t rm_compare_blocks_per_frame(int64_t npx, int32_t n_frames);
hipError_t rm_launch_compare(const RmCompareArgs &a, int32_t map, int32_t n_frames, int32_t blocks_per_frame, hipStream_t stream,
                             const char **kernel_name);

// rm_counter_hist_device: ONE launch of hist_kernel<masked> over n_frames frames of a.npx pixels (0 included), blocks_per_frame
// workgroups each (rm_compare_blocks_per_frame: the same shape); a.scratch holds one entry per frame when blocks_per_frame > 1.
hipError_t rm_launch_hist(const RmHistArgs &a, bool masked, int32_t n_frames, int32_t blocks_per_frame, hipStream_t stream,
                          const char **kernel_name);
// rm_shade_ranged_device: ONE launch of shade_ranged_kernel; nothing without a pixel or a frame.
hipError_t rm_launch_shade_ranged(const RmShadeRangedArgs &a, int32_t n_frames, hipStream_t stream, const char **kernel_name);
// rm_shade_lit_device: ONE launch of shade_lit_kernel; nothing without a pixel or a frame.
hipError_t rm_launch_shade_lit(const RmShadeLitArgs &a, int32_t n_frames, hipStream_t stream, const char **kernel_name);
// rm_shade_field_device: ONE launch of shade_field_kernel; nothing without a value.
hipError_t rm_launch_shade_field(const RmShadeFieldArgs &a, hipStream_t stream, const char **kernel_name);

hipError_t rm_launch_hypot(const float *xyz, int64_t n, double *out, hipStream_t stream);
// rm_jsmath.h on the device: fn 0 sin, 1 cos, 2 atan2, 3 asin, 4 log, 5 pow, 6 round, 7 atan
hipError_t rm_launch_jsmath(int fn, const double *a, const double *b, int64_t n, double *out, hipStream_t stream);

// compares the two device forms of Math.hypot on n generated triples; adds mismatches
hipError_t rm_launch_fastdiv_selftest(uint64_t seed, int64_t n, unsigned long long *d_mismatches, hipStream_t stream);
hipError_t rm_launch_recip_selftest(int mode, unsigned long long *d_mismatches, hipStream_t stream);
#endif  // !__HIPCC_RTC__
