/*
 * rm_raymarch.h -- C ABI of the MI355X-native sphere-tracing render path.
 *
 * Drop-in boundary for ONE path of vxlerian/cpu-raymarcher: the per-pixel render path
 *   worker tile dispatch -> Raymarcher.runRaymarcher -> SphereTracer.rayMarch
 *   -> BVH / Octree callbacks -> Scene.getDistance -> Sphere.sdf, then ShadingModel.shade
 * (reference files cited per entry point, paths relative to the reference's src/).
 *
 * Plain pointers and sizes only; no C++/torch types.  Every function returns an
 * rm_status (0 = ok, negative = error) unless stated; nothing throws or aborts across
 * the boundary (the reference has no error path on this route: bad inputs are clamped
 * or defaulted exactly as the reference does, see each entry).
 *
 * Buffers follow the reference's typed arrays (raymarchWorker.ts:42-46):
 *   depth  : uint8  [W*h]      Uint8ClampedArray
 *   normal : uint8  [W*h*3]    Uint8ClampedArray, RGB interleaved
 *   sdf    : uint16 [W*h]      Uint16Array  (SDF evaluations per pixel, wraps mod 65536)
 *   iters  : uint16 [W*h]      Uint16Array  (march iterations per pixel)
 *   rgba   : uint8  [W*h*4]    Uint8ClampedArray (ImageData)
 * all tile-local, row-major, h = max(0, yEnd - yStart).  The caller owns every buffer;
 * the library never frees or retains one (the reference transfers ownership back to the
 * main thread, raymarchWorker.ts:86-91).
 *
 * Threading: an rm_ctx is bound to one GPU and is not thread-safe; use one ctx per host
 * thread / GPU (the reference keeps one job in flight per worker, main.ts:447-490).
 */
#ifndef RM_RAYMARCH_H
#define RM_RAYMARCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_API __attribute__((visibility("default")))

typedef struct rm_ctx rm_ctx;

typedef enum rm_status {
    RM_OK = 0,
    RM_E_INVALID = -1,     /* null pointer, negative size, non-finite camera ...            */
    RM_E_UNSUPPORTED = -2, /* valid request the native path cannot serve (operator tree     */
                           /* nested deeper than 15, BVH leaf above 255 primitives): the    */
                           /* host keeps its own CPU path for that job                      */
    RM_E_NO_DEVICE = -3,   /* ctx was created host-only, or no HIP device                   */
    RM_E_HIP = -4,         /* a HIP runtime call failed; rm_last_error has the text         */
    RM_E_NO_SCENE = -5,    /* render requested before any scene was set                     */
    RM_E_NOMEM = -6
} rm_status;

/* Scene.accelerationStructure strings "None" | "Octree" | "BVH" (scene.ts:21,32-36) */
typedef enum rm_accel { RM_ACCEL_NONE = 0, RM_ACCEL_OCTREE = 1, RM_ACCEL_BVH = 2 } rm_accel;

/* Job.algorithm strings (raymarchWorker.ts:50-68) */
typedef enum rm_algorithm {
    RM_ALG_SPHERE_TRACER = 0, /* 'sphere-tracer' and every unknown string (default branch) */
    RM_ALG_FIXED_STEP = 1,
    RM_ALG_ADAPTIVE_STEP = 2,
    RM_ALG_ADAPTIVE_STEP_V2 = 3,
    RM_ALG_ADAPTIVE_STEP_V3 = 4
} rm_algorithm;

/* shading model strings (main.ts:33-45) */
typedef enum rm_shader {
    RM_SHADE_NORMAL = 0, /* 'normal' and every unknown string */
    RM_SHADE_PHONG = 1,
    RM_SHADE_SDF_HEATMAP = 2,
    RM_SHADE_ITERATION_HEATMAP = 3
} rm_shader;

/* scene_preset_index value that selects the scene last given to rm_scene_from_spheres */
#define RM_SCENE_UPLOADED INT32_MIN

/* Replaces the worker message `Job` (raymarchWorker.ts:10-22).  The reference worker
 * rebuilds the scene from (scenePresetIndex, accelerationStructure) for every job
 * (raymarchWorker.ts:37-38); here the ctx caches the built, device-resident scene and
 * rebuilds only when those two fields change. */
typedef struct rm_job {
    int32_t width;                  /* Job.width  : full-frame width                     */
    int32_t height;                 /* Job.height : full-frame height                    */
    double  time;                   /* Job.time   : unused by sphere primitives          */
    int32_t y_start;                /* Job.yStart                                        */
    int32_t y_end;                  /* Job.yEnd   (rows [y_start, y_end))                */
    double  camera_pitch;           /* Job.camera.pitch (clamped to +-pi/2, camera.ts:59) */
    double  camera_yaw;             /* Job.camera.yaw                                    */
    int32_t algorithm;              /* rm_algorithm                                      */
    int32_t scene_preset_index;     /* clamped to [0, 18] (scene.ts:39) or RM_SCENE_UPLOADED */
    int32_t acceleration_structure; /* rm_accel                                          */
    int32_t reserved;
    double  overshoot_factor;       /* Job.overshootFactor, AdaptiveStepV2/V3; NaN = JS undefined -> 1.2 */
    double  step_size;              /* Job.stepSize, FixedStep;               NaN = JS undefined -> 0.1 */
} rm_job;

/* what rm_scene_get_info reports about the built acceleration structure */
typedef struct rm_scene_info {
    int32_t n_prims;
    int32_t accel;           /* rm_accel */
    int32_t preset_index;    /* or RM_SCENE_UPLOADED */
    int32_t bvh_nodes, bvh_leaves, bvh_depth;
    int32_t oct_nodes, oct_leaves, oct_empty_leaves, oct_max_leaf_prims;
    float   root_min[3], root_max[3];
    int32_t nodes_in_lds;    /* 1 when the flattened node table is staged in LDS */
    int32_t program;         /* expression forests: what the interpreter's program needs, position slots | pending values << 8 |
                                instructions << 16 (accepted: up to 15 slots -- one fewer than RM_PROG_MAX_SLOTS, a node at
                                slot s may write slot s + 1 --, up to 16 values, (slots * 12 + values * 8) * 256 <= 64 KiB); else 0 */
} rm_scene_info;

/* diagnostics of main.ts:528-548 */
typedef struct rm_diagnostics {
    uint64_t total_sdf_calls;
    uint64_t total_iterations;
    uint32_t max_sdf_calls;
    uint32_t min_sdf_calls;  /* Number.MAX_SAFE_INTEGER in the reference when n == 0; UINT32_MAX here */
    uint64_t total_pixels;
} rm_diagnostics;

/* ---- context ------------------------------------------------------------------- */

/* device >= 0: bind to that HIP device.  device == -1: host-only ctx (scene building and
 * camera only; every render entry returns RM_E_NO_DEVICE).  There is no CPU fallback. */
RM_API int rm_create(int device, rm_ctx **out);
RM_API void rm_destroy(rm_ctx *ctx);
RM_API const char *rm_last_error(const rm_ctx *ctx); /* never NULL */
/* the render-kernel instantiation the most recent render entry launched ("" before the first; never NULL):
 * measurement aid, so that a benchmark line names the kernel that really ran */
RM_API const char *rm_last_kernel(const rm_ctx *ctx);
RM_API const char *rm_version(void);

/* string -> enum with the reference's defaulting rules (never fail) */
RM_API int rm_algorithm_from_string(const char *s); /* raymarchWorker.ts:50-68 */
RM_API int rm_accel_from_string(const char *s);     /* scene.ts:32-36          */
RM_API int rm_shader_from_string(const char *s);    /* main.ts:33-45           */
RM_API int rm_preset_count(void);                   /* sceneManager.ts:363-365 */

/* ---- scene --------------------------------------------------------------------- */

/* Replaces `new Scene(accel); scene.loadPreset(index)` (scene.ts:24-59,
 * raymarchWorker.ts:37-38): builds the primitive list, the BVH (bvh.ts:29-92) or Octree
 * (octree.ts:36-191), flattens it and uploads it.  All 19 presets are native: 0..4 (spheres),
 * 5, 7, 8, 9 (torus, boxes), 6 and 10..18 (SDF operators, Mandelbulb; index clamps like
 * sceneManager.ts:359-361). */
RM_API int rm_scene_from_preset(rm_ctx *ctx, int32_t preset_index, int32_t accel);

/* Build-defined scene entry: n spheres as SceneManager.createSphere(x, y, z, r) without
 * rotation would make them (sceneManager.ts:21-41): centre f32, radius a double
 * (sphere.ts:5-9).  Selected in jobs by scene_preset_index = RM_SCENE_UPLOADED. */
RM_API int rm_scene_from_spheres(rm_ctx *ctx, const float *centers_xyz, const double *radii,
                                 int32_t n, int32_t accel);

/* Edits the active sphere scene in place: the "update" of object CRUD beside rm_ray_pick (which object) and rm_scene_object
 * (read it back).  The active scene must be a sphere list -- one given to rm_scene_from_spheres, or preset 0..4.  Its objects,
 * in object order (what rm_ray_pick and rm_scene_object index by, never a device slot), form a list, and the edits apply to
 * that list in order: SET replaces entry index (0 <= index < n), INSERT puts a new sphere before index (0 <= index <= n),
 * REMOVE deletes entry index; n is the list's length when the edit's turn comes.  Afterwards the context is in every observable
 * respect what rm_scene_from_spheres(ctx, edited list, the active acceleration structure) leaves: the scene is the uploaded
 * one (RM_SCENE_UPLOADED in jobs and in rm_scene_get_info, also when a preset was edited), a job that names another
 * acceleration structure rebuilds the edited list, and every render, query, pick, object index and device table is
 * bit-identical.  All or nothing: the whole list of edits is checked before anything changes, and on any error the scene, its
 * device tables and the remembered upload are as before.
 *   RM_E_INVALID      null edits with n_edits > 0, n_edits < 0, an op outside the enum, reserved != 0, a non-finite centre
 *                     or radius in SET / INSERT (all checked ahead of everything else), an index out of range at its turn
 *   RM_E_NO_SCENE     before any scene
 *   RM_E_UNSUPPORTED  the active scene is a primitive list, a forest or preset 5..18: those keep no candidate tables and
 *                     rebuild in milliseconds; rm_scene_object -> rm_scene_from_nodes stays their route
 *   a build error of the edited list is reported as rm_scene_from_spheres reports it.
 * n_edits == 0 (on a scene that could be edited) is RM_OK, rebuilds nothing and leaves a preset a preset.
 * What makes the edit cheaper than an upload: with option device_build = 1 (default) and a device, the four (cell, sphere) /
 * (node, box) pair loops of the build -- the BVH's nearest-candidate grid and exterior candidate grid, the sub-cell lists of
 * crowded octree leaves, the empty octree nodes' distance to the nearest primitive box -- run as HIP kernels
 * (csrc/rm_scene_build.hip) that repeat the host's binary64 arithmetic operation for operation; trees, leaf grid and cell
 * table stay on the host.  A table whose lists would reach 2^24 entries (there the host's rule depends on the order of
 * the cells), or whose device build fails, is built by the host loop instead: same bytes.  device_build = 0, or a host-only
 * context: the host builder for everything.  The upload entries never read the option.
 * Synchronises the device like every scene upload.  Not a render entry: it neither consumes nor fires
 * rm_render_attach_diagnostics, and leaves rm_last_kernel's answer and rm_scene_set_time's value alone. */
typedef enum rm_edit_op { RM_EDIT_SET = 0, RM_EDIT_INSERT = 1, RM_EDIT_REMOVE = 2 } rm_edit_op;
typedef struct rm_sphere_edit {   /* 32 bytes */
    int32_t op;          /* rm_edit_op */
    int32_t index;       /* object index at the moment this edit applies */
    float   center[3];   /* SET, INSERT; ignored by REMOVE */
    int32_t reserved;    /* 0 */
    double  radius;      /* SET, INSERT; a double, as rm_scene_from_spheres takes it */
} rm_sphere_edit;
RM_API int rm_scene_edit_spheres(rm_ctx *ctx, const rm_sphere_edit *edits, int32_t n_edits);

/* General primitives: Sphere / Box / Torus with any world->local matrix
 * (primitives/sphere.ts, box.ts, torus.ts; Primitive.sdf primitive.ts:33-39). */
typedef enum rm_prim_type { RM_PRIM_SPHERE = 0, RM_PRIM_BOX = 1, RM_PRIM_TORUS = 2 } rm_prim_type;
typedef struct rm_prim {
    int32_t type;               /* rm_prim_type */
    int32_t reserved;
    float   world_to_local[16]; /* Primitive.transform, gl-matrix layout (column-major) */
    double  params[3];          /* sphere: radius; box: halfSize x,y,z (stored f32, box.ts:10); */
                                /* torus: majorRadius, minorRadius                               */
    double  reserved2;
} rm_prim;

/* n primitives of any of the three kinds, selected in jobs by RM_SCENE_UPLOADED. */
RM_API int rm_scene_from_prims(rm_ctx *ctx, const rm_prim *prims, int32_t n, int32_t accel);

/* SceneManager.getTransform(x, y, z, rotation?) (sceneManager.ts:21-37): the world->local
 * matrix of a primitive; rotation_xyz may be NULL (no rotation argument) or three Euler
 * angles stored as binary32 like a gl-matrix vec3. */
RM_API int rm_make_transform(double x, double y, double z, const float *rotation_xyz, float *world_to_local16);

/* SDF expression forests: the operator classes of util/primitive_operations/
 * (round.ts, smoothUnion.ts, smoothSubstraction.ts, twist.ts, repetition.ts, animatedTranslate.ts)
 * over Sphere / Box / Torus / Mandelbulb (primitives/mandelbulb.ts) leaves.  All 19 presets of
 * sceneManager.ts:102-357 are served natively through rm_scene_from_preset / rm_job; this entry
 * takes an arbitrary forest.  Operands must precede the node that uses them. */
typedef enum rm_node_type {
    RM_NODE_SPHERE = 0, RM_NODE_BOX = 1, RM_NODE_TORUS = 2, RM_NODE_MANDELBULB = 3,
    RM_NODE_ROUND = 10, RM_NODE_SMOOTH_UNION = 11, RM_NODE_SMOOTH_SUBTRACTION = 12,
    RM_NODE_TWIST = 13, RM_NODE_REPETITION = 14, RM_NODE_ANIMATED_TRANSLATE = 15
} rm_node_type;
typedef struct rm_node {
    int32_t type;               /* rm_node_type */
    int32_t child_a, child_b;   /* operand node indices (< own index); -1 when unused */
    int32_t reserved;
    float   world_to_local[16]; /* leaves: Primitive.transform.  Operators derive theirs as their
                                 * constructors do (wrappers: the operand's; unions: identity) */
    double  params[6];          /* sphere: radius | box: halfSize | torus: major, minor |
                                 * mandelbulb: power, iterations, enableAnimation, animationSpeed |
                                 * round: radius | unions: smoothness | twist: twistAmount |
                                 * repetition: spacing x,y,z | animated translate: the NORMALISED
                                 * direction x,y,z (animatedTranslate.ts:22-23), amplitude, speed */
} rm_node;

/* roots[] lists the nodes that are Scene.objects, in order; selected in jobs by RM_SCENE_UPLOADED.
 * RM_E_UNSUPPORTED when a tree is deeper than the device interpreter's 15 nested operators. */
RM_API int rm_scene_from_nodes(rm_ctx *ctx, const rm_node *nodes, int32_t n_nodes, const int32_t *roots,
                               int32_t n_roots, int32_t accel);

/* gl-matrix mat4.scale(m, m, [x, y, z]) in place: SceneManager.createMandelbulb post-scales the
 * world->local matrix by 0.5 (sceneManager.ts:63). */
RM_API int rm_scale_transform(float *world_to_local16, double x, double y, double z);

/* Scene.updateTime(time) (scene.ts:135-140) for rm_scene_distance; renders take rm_job.time. */
RM_API int rm_scene_set_time(rm_ctx *ctx, double time);

RM_API int rm_scene_get_info(const rm_ctx *ctx, rm_scene_info *out);

/* Camera.setAngles + getRotationMatrix/getPosition (camera.ts:38-44,58-69,81-88):
 * writes mat3.fromMat4 of the rotation (9 floats, column-major) and the origin. */
RM_API int rm_camera_from_angles(double pitch, double yaw, float *rot9, float *origin3);

/* Scene.getDistance(position, counter) (scene.ts:144-190) for a batch of points, on the
 * device: dist[i] and count[i] (primitives evaluated) for points xyz f32[3n] (host). */
/* Test entry: the same query for a BVH sphere scene through the distance function of the v2 wave loop (one point per lane, every
 * option -- filter, grid, nn, ext, uniform, coop -- as in a render of the scene; csrc/rm_render_v2.hip bvh_distance_wave).  Same
 * values and counts as rm_scene_distance, bit for bit; RM_E_UNSUPPORTED for any other scene. */
RM_API int rm_debug_wave_distance(rm_ctx *ctx, const float *points_xyz, int64_t n, double *dist, uint32_t *count);
RM_API int rm_scene_distance(rm_ctx *ctx, const float *points_xyz, int64_t n, double *dist,
                             uint32_t *count);

/* ---- field queries: distance slices and volumes sampled on the device ------------------- */

typedef struct rm_lattice {      /* 72 bytes */
    float   origin[3];           /* point (0, 0, 0) */
    float   du[3], dv[3], dw[3]; /* step per index i, j, k */
    int32_t nu, nv, nw;          /* points along i, j, k: each 0 .. 65535 */
    int32_t reserved;            /* 0 */
    double  time;                /* Scene.updateTime for this query; rm_scene_set_time's value is kept */
} rm_lattice;

/* Scene.getDistance (scene.ts:144-190) at the n = nu * nv * nw points of a lattice the device forms itself: a plane through
 * the scene (nw = 1) for a slice image, a volume for a mesher, a collision grid or a 3D texture -- 72 bytes go up instead of
 * 12 per point.  The rule:
 *   index   point (i, j, k), 0 <= i < nu, 0 <= j < nv, 0 <= k < nw, has the linear index (k * nv + j) * nu + i, a 64-bit value;
 *           every output is indexed by it.
 *   point   component c of point (i, j, k) is
 *             f32((((double)origin[c] + (double)i * (double)du[c]) + (double)j * (double)dv[c]) + (double)k * (double)dw[c]):
 *           binary64 arithmetic, left to right, no contraction (no fused multiply-add), ONE rounding to binary32 at the end.
 *           rm_lattice_points writes exactly these points on the host.
 *   value   dist[l] and count[l] are what rm_scene_distance returns for that point with Scene.updateTime(lattice->time):
 *           the same distance function the renders and the ray queries call, the primitives it counted; dist32[l] is
 *           (float)dist[l].  getDistance is taken as it is: an empty octree leaf answers minDistance * 0.99, the minimum starts
 *           at 10, a point in no BVH leaf box is measured against every primitive -- a field under a BVH or an octree is the
 *           bound the marchers walk through, not always the exact distance, and a slice of it shows where.  Option `exact`
 *           (below) answers the exact field E instead; count is then the evaluations made.
 * Each of dist (f64[n]), dist32 (f32[n]) and count (u32[n]) may be NULL.  RM_E_INVALID -- like every argument check ahead of
 * RM_E_NO_DEVICE and RM_E_NO_SCENE, and also when a count is 0 -- for a null lattice, a count outside 0 .. 65535,
 * reserved != 0, a non-finite origin, step or time, a non-finite binary32 component at any of the lattice's eight corner points
 * (indices 0 and count - 1, 0 on an axis without points; each component is monotone in each index, so the corners bound every
 * point), a dist that is not 8-byte or a dist32 / count that is not 4-byte aligned, and all three outputs NULL with n > 0.  A
 * lattice with a zero count has n = 0: RM_OK, nothing is launched or written.
 * Not a render entry: it neither consumes nor fires rm_render_attach_diagnostics and leaves rm_scene_set_time's value
 * alone; knobs apply as for rm_scene_distance (`filter`, `length`).  Scenes whose renders run a run-time specialised kernel
 * are served by the ahead-of-time kernels here (same values).  rm_last_kernel names the field_kernel<ACCEL, GEN>
 * instantiation.  Host buffers, synchronous, chunked through the context's scratch buffer: a chunk is a set of whole lattice
 * rows (runs of nu points) of at most 4 M points -- one row when nu alone is more --, and only the outputs asked for are staged
 * and copied back. */
RM_API int rm_scene_field(rm_ctx *ctx, const rm_lattice *lattice, double *dist, float *dist32, uint32_t *count);

/* Same with device pointers, asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream), as
 * rm_ray_march_device: one launch for up to 2^30 points. */
RM_API int rm_scene_field_device(rm_ctx *ctx, const rm_lattice *lattice, void *d_dist, void *d_dist32, void *d_count, void *stream);

/* The points of linear indices [first, first + n) of a lattice by the rule above (f32[3n]), host-only, no ctx:
 * rm_scene_distance over them is by definition what the field query returns.  RM_E_INVALID for a lattice rm_scene_field
 * refuses, first < 0, n < 0, first + n > nu * nv * nw or null points_xyz with n > 0. */
RM_API int rm_lattice_points(const rm_lattice *lattice, int64_t first, int64_t n, float *points_xyz);

/* ---- meshes: the surface of a distance volume, extracted on the device (naive surface nets) ------------------- */

typedef struct rm_mesh_info {    /* 32 bytes */
    int64_t n_vertices;          /* active cells: the true total, also when it exceeds the capacity */
    int64_t n_quads;             /* likewise */
    int64_t n_holes;
    int64_t reserved;            /* written 0 */
} rm_mesh_info;
enum { RM_MESH_F64 = 0, RM_MESH_F32 = 1 };

/* Surface nets over the values of a lattice: one vertex per cell the surface passes through, one quad per lattice edge whose
 * ends lie on different sides.  The rule, operation for operation (tests/mesh_model.py restates it; results are equal byte
 * for byte):
 *   input     an rm_lattice (as rm_scene_field takes and checks it), one value per point at its linear index
 *             l = (k * nv + j) * nu + i, binary64 or binary32 (widened: exact), and a binary64 `iso`.
 *   inside    point l is inside iff value[l] < iso: NaN is outside, a value equal to iso is outside, -0.0 < 0.0 is false.
 *   cells     cell (i, j, k), 0 <= i < nu - 1, 0 <= j < nv - 1, 0 <= k < nw - 1, has its corners at offsets (dx, dy, dz) in
 *             {0, 1}^3.  It is ACTIVE iff all eight corner values are finite and the corners are neither all inside nor all
 *             outside; a HOLE iff they are neither all inside nor all outside and a corner value is not finite: a hole emits
 *             nothing and is counted.  A lattice with a count below 2 has no cells.
 *   vertices  active cells are numbered 0, 1, 2, ... by the linear index of their low corner; that number is the vertex index.
 *   position  visit the cell's twelve edges: axis A = 0, 1, 2, and within an axis the edge's low corner at offsets (0,0), (1,0),
 *             (0,1), (1,1) on the other two axes, the lower-numbered axis first.  With a the value at the edge's low end and b
 *             at its high end: if exactly one end is inside, t = (iso - a) / (b - a), the crossing's local coordinates are t on
 *             axis A and the 0 / 1 offsets on the other two; add the three to three running sums that start at 0.0 and count
 *             the crossing in m.  f = sum / (double)m per axis, and component c of the vertex is
 *               f32((((double)origin[c] + ((double)i + f[0]) * (double)du[c]) + ((double)j + f[1]) * (double)dv[c])
 *                   + ((double)k + f[2]) * (double)dw[c]):
 *             binary64, left to right, one operation at a time, no contraction, ONE rounding to binary32 -- the lattice's own
 *             point rule with a fractional index.  Vertices are float[3].
 *   quads     every lattice edge from point p = (i, j, k) along axis A to p + e_A whose ends differ in `inside`: with (B, C) the
 *             other two axes in cyclic order (A = 0: (1, 2); 1: (2, 0); 2: (0, 1)) the four cells around it have their low
 *             corners at c0 = p - e_B - e_C, c1 = p - e_C, c2 = p, c3 = p - e_B.  The edge emits a quad iff all four cells
 *             exist and are active: (v(c0), v(c1), v(c2), v(c3)) when p is inside -- counter-clockwise seen from +A in index
 *             space, the normal points out of the inside --, (v(c0), v(c3), v(c2), v(c1)) when p is outside.  Quads are
 *             uint32[4], in increasing 3 * l(p) + A.
 *   winding   is defined in index space: a lattice whose (du, dv, dw) is left-handed gets world-space normals that point
 *             inwards.  The Python helpers flip the winding then; this ABI does not.
 * Capacities: nothing is written at or beyond a capacity; `info` always holds the true totals; a capacity of 0 with a null
 * buffer is the counting call (it runs the count and the scan alone); truncation is RM_OK -- compare totals with capacities --,
 * vertex r < cap_vertices and quad q < cap_quads are exactly what an untruncated call writes there, and a truncated quad list
 * may name vertices >= cap_vertices.
 *
 * rm_mesh_field_device: values already on the device (rm_scene_field_device's dist or dist32, or anything else laid out by
 * the lattice; lattice->time is not used), outputs and d_info (an rm_mesh_info) on the device, asynchronous on `stream` as
 * rm_scene_field_device: four kernels, no host round trip.  It needs no scene.  RM_E_INVALID -- ahead of RM_E_NO_DEVICE --
 * for everything rm_scene_field refuses about a lattice, more than 2^30 points (the mesher does not split a volume), null
 * d_values when the lattice has cells, null d_info, a non-finite iso, a value_type outside the enum, a negative capacity, a
 * null buffer with a capacity above 0, vertices or quads not 4-byte aligned, d_info or binary64 values not 8-byte aligned
 * (binary32 values: 4).  A lattice without cells is RM_OK: zero totals, nothing launched.
 * The cell -> vertex map (4 bytes per point) and the workgroup totals live in the context's scratch buffer.  Calls that use
 * the scratch are ordered on the device, whatever their streams: the next one waits for this call's kernels.  When the
 * scratch has to grow the device is synchronised first, so that one call is not asynchronous.
 * Not a render entry: it neither consumes nor fires rm_render_attach_diagnostics and leaves rm_scene_set_time's value alone;
 * like rm_scene_field it names its own kernel in rm_last_kernel: mesh_count_kernel<double> or <float>, the first of the four. */
RM_API int rm_mesh_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso,
                                void *d_vertices, int64_t cap_vertices, void *d_quads, int64_t cap_quads, void *d_info, void *stream);

/* Samples the ACTIVE scene on the lattice at lattice->time (the launch of rm_scene_field_device, binary64, into the context's
 * scratch buffer) and meshes the volume, all on the device; host buffers, synchronous: min(total, capacity) vertices and quads
 * are copied back.  The same checks without d_values and value_type (no alignment is asked of `info`), and RM_E_NO_SCENE last.
 * The scratch holds 12 bytes per point plus the outputs up to their capacities.  A field under a BVH or an octree is the
 * marchers' bound, not always the exact distance: exact offset surfaces (iso != 0) want option `exact` (below). */
RM_API int rm_scene_mesh(rm_ctx *ctx, const rm_lattice *lattice, double iso, float *vertices, int64_t cap_vertices,
                         uint32_t *quads, int64_t cap_quads, rm_mesh_info *info);

/* ---- sparse meshes: the same mesh from the 8 x 8 x 8-cell blocks near the surface ------------------------------ */

#define RM_SPARSE_BLOCK 8
typedef struct rm_sparse_info {  /* 32 bytes */
    int64_t n_blocks;            /* blocks of the lattice */
    int64_t n_kept;              /* blocks the coarse pass kept */
    int64_t reserved[2];         /* written 0 */
} rm_sparse_info;

/* Only a thin shell of cells around the surface can hold a vertex, and a distance says how far the surface is: one exact
 * evaluation per block proves most of a volume empty.  Three device entries in the style of the dense path -- the caller owns
 * every buffer, counting and filling calls are asynchronous -- and one host convenience entry.  The rule, operation for
 * operation (tests/mesh_sparse_model.py restates it; results are equal byte for byte):
 *   blocks    B = RM_SPARSE_BLOCK = 8.  An axis with n points has ceil((n - 1) / 8) blocks, 0 when n < 2 (rm_lattice_blocks).
 *             Block (bx, by, bz) has the linear index (bz * nbv + by) * nbu + bx; its cells are 8 bx .. min(8 bx + 8, nu - 1) - 1
 *             on axis i and likewise on j and k.  At most 2^24 blocks; the 2^30-point limit of the dense mesher does not
 *             apply, counts up to 65 535 per axis are allowed, fine linear indices are 64-bit values everywhere.
 *   tile      the 9 x 9 x 9 lattice points (8 bx + a, 8 by + b, 8 bz + g), a, b, g = 0 .. 8, of a block; the value of tile
 *             point (a, b, g) sits at (g * 9 + b) * 9 + a.  A tile point beyond the lattice holds the quiet NaN
 *             0x7FF8000000000000; no existing cell reads it.
 *   centre    of a block: the lattice point (min(8 bx + 4, nu - 1), min(8 by + 4, nv - 1), min(8 bz + 4, nw - 1)), formed by
 *             the lattice's own point rule (binary64, left to right, one rounding to binary32).
 *   d         the EXACT field at the centre at lattice->time: min(10, min over all objects of Primitive.sdf) -- what
 *             rm_scene_distance returns for an acceleration-None upload of the same scene, byte for byte, whatever
 *             acceleration the active scene has.  (A BVH or octree field is the marchers' bound; under a BVH it is an
 *             over-estimate and cannot prove a block empty.)  Under a BVH, sphere and primitive-record scenes find d by a
 *             pruned walk of the skip-linked nodes: best starts at 10; with db the binary64 distance from the centre to a
 *             node's box (0 inside), sqrt((ex * ex + ey * ey) + ez * ez) of the per-axis excesses, the subtree is skipped iff
 *             db * (1 - 2^-20) - 2^-20 > best; at a leaf best = min(best, Primitive.sdf) for each of its primitives.  A
 *             primitive lies inside its leaf's box, so the pruned minimum is the full minimum.  Every other scene evaluates
 *             every object.
 *   bound     R = 4 * (|du| + |dv| + |dw|), each norm sqrt((x * x + y * y) + z * z) in binary64 of the widened binary32 step:
 *             no point of a block's cells is farther from its centre.  slack = M * 2^-20, M the largest |component| among the
 *             lattice's eight binary32 corner points (indices 0 and count - 1): it covers the binary32 rounding of two points.
 *             bound = lipschitz * R + slack, binary64, in that order.
 *   keep      a block is KEPT iff !(fabs(d - iso) > bound): a NaN distance keeps the block.
 *             GUARANTEE: if the exact field is `lipschitz`-Lipschitz (every distance function of primitives and of unions is
 *             1-Lipschitz; smooth blends and displacements may need more), no dropped block contains a point where
 *             field - iso changes sign.
 *   slots     kept blocks are numbered 0, 1, 2, ... in increasing block index: the block's slot.
 *   mesh      inside / active / hole, the vertex position, the quad ring and the winding are rm_mesh_field_device's rule
 *             unchanged, on the tile values, except: a cell of a block that was not kept is not active, and holes are counted
 *             in kept blocks only.  Vertices are numbered by (slot, local cell index (z * 8 + y) * 8 + x); quads are in
 *             increasing (slot of the block whose cell has its low corner at p, 3 * local(p) + A).
 *   keys      cells[v] is the fine linear index l = (k * nv + j) * nu + i of vertex v's cell, edges[q] is 3 * l(p) + A of quad
 *             q: the dense mesher's sort keys.  Sorting the vertices by cells and the quads by edges (and renaming the
 *             vertices) gives rm_mesh_field_device's mesh of the same values, byte for byte, whenever every cell that is
 *             active in the dense volume lies in a kept block.
 *
 * rm_lattice_blocks: the three block counts of a lattice, host-only, no ctx; RM_E_INVALID for a lattice rm_scene_field
 * refuses or null dims.
 *
 * rm_scene_blocks_device: which blocks to keep, one lane per block; a count kernel, a scan and a scatter, asynchronous on
 * `stream`, nothing depends on arrival order.  d_slot int32[n_blocks]: the block's slot or -1.  d_list int32[n_blocks]: the
 * kept blocks in slot order (entries from n_kept on are not written).  d_dist f64[n_blocks], optional: d per block.  d_info:
 * an rm_sparse_info.  RM_E_INVALID -- ahead of RM_E_NO_DEVICE, and RM_E_NO_SCENE last -- for everything rm_scene_field
 * refuses about a lattice, more than 2^24 blocks, a non-finite iso, a lipschitz that is not finite and > 0, null d_info, null
 * d_slot or d_list when the lattice has blocks, d_slot / d_list not 4-byte or d_dist / d_info not 8-byte aligned.  A lattice
 * without blocks is RM_OK: zero info, nothing launched.  rm_last_kernel: blocks_kernel<GEN, WALK>.
 *
 * rm_scene_tiles_device: the ACTIVE scene's own distance function -- the values rm_scene_field returns, bit for bit -- at the
 * 729 points of each of the n_kept blocks of d_list, into d_tiles f64[n_kept][729].  One 256-thread workgroup per kept block,
 * three passes, a fastest: a wave's points sit in one small box, so its BVH candidates are coherent.  Faces shared by two kept
 * blocks are evaluated once per block that touches them: 729 evaluations against 512 points of a block's own.  Ahead-of-time
 * kernels only; the knobs `filter` and `length` apply as for rm_scene_field.  RM_E_INVALID for the lattice as above, n_kept
 * outside 0 .. n_blocks, a null d_list or d_tiles with n_kept > 0, d_list not 4-byte or d_tiles not 8-byte aligned;
 * RM_E_NO_DEVICE; RM_E_NO_SCENE last.  n_kept == 0 is RM_OK.  rm_last_kernel: tiles_kernel<ACCEL, GEN>.  With option `exact`
 * (below) the tiles hold the exact field E -- what the coarse pass decided by -- instead, for offset surfaces and octree scenes.
 *
 * rm_mesh_tiles_device: surface nets over the tiles; it needs no scene, like rm_mesh_field_device.  One workgroup per kept
 * block, the tile staged once in LDS, two cells per lane; neighbour blocks are reached through d_slot; a cell -> vertex map
 * (2 KB per kept block) and the workgroup totals live in the context's scratch buffer, ordered as rm_mesh_field_device's.
 * d_cells (int64 per vertex) and d_edges (int64 per quad) are optional and sized by the capacities.  The counting and
 * capacity protocol, the truncation semantics and rm_mesh_info are exactly rm_mesh_field_device's.  RM_E_INVALID for the
 * lattice as above, n_kept outside 0 .. min(n_blocks, 2^21) (vertex numbers are 32-bit), null d_info, null d_slot when the
 * lattice has blocks, null d_list or d_tiles with n_kept > 0, a non-finite iso, a negative capacity, a null vertex or quad
 * buffer with a capacity above 0, d_slot / d_list / vertices / quads not 4-byte or d_tiles / d_cells / d_edges / d_info not
 * 8-byte aligned; RM_E_NO_DEVICE.  n_kept == 0 is RM_OK: zero totals.  rm_last_kernel: mesh_tiles_count_kernel.
 *
 * rm_scene_mesh_sparse: the three steps in the context's scratch buffer with n_kept read back once in between; host buffers,
 * synchronous: min(total, capacity) vertices, quads and keys are copied back.  cells, edges and sparse_info may be NULL.  The
 * checks of the three entries for its own arguments (no alignment is asked of info and sparse_info), ahead of RM_E_NO_DEVICE;
 * RM_E_NO_SCENE last; RM_E_UNSUPPORTED when more than 2^21 blocks are kept (sparse_info says how many).  The scratch holds 8
 * bytes per block, and per kept block its tile and its map, plus the outputs up to their capacities.  None of the four is a render entry: they neither consume nor fire rm_render_attach_diagnostics and
 * leave rm_scene_set_time's value alone. */
RM_API int rm_lattice_blocks(const rm_lattice *lattice, int32_t dims[3]);
RM_API int rm_scene_blocks_device(rm_ctx *ctx, const rm_lattice *lattice, double iso, double lipschitz, void *d_slot, void *d_list,
                                  void *d_dist, void *d_info, void *stream);
RM_API int rm_scene_tiles_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_list, int64_t n_kept, void *d_tiles, void *stream);
RM_API int rm_mesh_tiles_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_slot, const void *d_list, int64_t n_kept,
                                const void *d_tiles, double iso, void *d_vertices, int64_t cap_vertices, void *d_quads, int64_t cap_quads,
                                void *d_cells, void *d_edges, void *d_info, void *stream);
RM_API int rm_scene_mesh_sparse(rm_ctx *ctx, const rm_lattice *lattice, double iso, double lipschitz, float *vertices, int64_t cap_vertices,
                                uint32_t *quads, int64_t cap_quads, int64_t *cells, int64_t *edges, rm_mesh_info *info,
                                rm_sparse_info *sparse_info);

/* ---- re-meshing an edited scene: only the tiles an edit can reach are sampled again ------------------------------
 *
 * The loop is pick -> edit -> look again.  After an edit the caller runs rm_scene_blocks_device afresh (one distance per block:
 * cheap, and it gives the new slot / list with no rule of its own), then rm_scene_tiles_update_device instead of
 * rm_scene_tiles_device, then rm_mesh_tiles_device as before.  The update is defined for the EXACT field E(x) = min(10, min over
 * all objects of Primitive.sdf(x)) only ("the exact field", below): a BVH or octree scene's own field changes everywhere when
 * an edit rebuilds the tree.  It does not read option `exact`: it IS the exact field.
 *
 * CONTRACT.  d_tiles afterwards holds, byte for byte, what rm_scene_tiles_device with option exact = 1 writes for the same
 * lattice, d_list and n_kept on the ACTIVE scene, given
 *   P1  d_prev_slot (int32[n_blocks]) and d_prev_tiles (f64[n_prev_kept][729]) are what the exact sparse path --
 *       rm_scene_blocks_device, then rm_scene_tiles_device with exact = 1 or this entry -- wrote for the PREVIOUS scene on the
 *       same lattice, `time` included;
 *   P2  the balls cover every object that differs between the two scenes, in each of its versions: for every such object
 *       version o there is a ball (c, rho) with Primitive.sdf_o(x) >= |x - c| - rho at every point x.  For a sphere: its own
 *       binary32 centre and its radius, with equality.  For a rigidly transformed box or torus: a ball that contains it.
 *       Objects whose index merely shifted are not changed objects: E does not depend on the order.
 * DECISION per kept block, b = d_list[r], the same for the 256 threads of its workgroup:
 *   1  p = d_prev_slot[b]; p outside 0 .. n_prev_kept - 1 (b outside 0 .. n_blocks - 1 counts as -1): EVALUATE.
 *   2  c = the tile's centre point as rm_scene_tiles_device forms it under exact: the lattice point rule at index 8 b + 4 per
 *      axis, NOT clamped to the lattice.  A non-finite component: EVALUATE.
 *   3  M = the largest of the previous tile's values at the tile points inside the lattice (i < nu, j < nv, k < nw; the NaN
 *      fill beyond it is skipped by index, not by value).  A NaN at a point inside the lattice: EVALUATE.
 *   4  for each ball, binary64, one operation at a time: lo = c - half, hi = c + half per axis, half the exact tile launch's
 *      own (4 (|du_a| + |dv_a| + |dw_a|) + slack, slack as under "bound" above); e = max(max(lo - cb, cb - hi), 0) per axis;
 *      gap = sqrt((ex * ex + ey * ey) + ez * ez); the ball REACHES the tile iff !(gap * (1 - 2^-20) - 2^-20 - rho > M) -- a
 *      NaN anywhere reaches.  Any ball that reaches: EVALUATE.
 *   5  otherwise COPY the 729 doubles of d_prev_tiles[p] to d_tiles[r].
 * EVALUATE is what rm_scene_tiles_device does for the block under exact, by the same device function.
 * WHY COPYING IS SOUND (DESIGN.md 4 has it in full).  The box c +- half contains every tile point, so a changed object
 * version's true lower bound at a tile point is gap - rho; the computed sdf falls below it by at most a relative 2^-23 of a
 * length (three binary32 roundings under a hypot), which the margins cover eight times over.  Hence every changed version has
 * sdf > M >= E_old at every tile point: no old version attains the old minimum, no new one can lower it, Math.min does not
 * depend on the order, and E_new and E_old are the same bits.  No Lipschitz assumption: the bound is the tile's own stored
 * values, so the rule holds for offset surfaces and deep inside large spheres.
 *
 * rm_scene_edit_balls: the balls of an edit list for rm_scene_edit_spheres, host-only (it works on a host-only context).  Call
 * it BEFORE rm_scene_edit_spheres with the same list: it replays the index bookkeeping on the active sphere list and writes,
 * in edit order, for SET the sphere before and after, for INSERT the new one, for REMOVE the old one -- at most 2 n_edits
 * balls.  *n_balls is their number whatever `cap` is; the first min(*n_balls, cap) are written (cap 0 and null balls: it only
 * counts).  RM_E_INVALID for null n_balls, cap < 0 or null balls with cap > 0; then it validates exactly as
 * rm_scene_edit_spheres does, same codes in the same order (after a refused index, balls written so far mean nothing and
 * *n_balls is 0).  It changes nothing.
 *
 * rm_scene_tiles_update_device: asynchronous on `stream`; one 256-thread workgroup per kept block (tiles_update_kernel<GEN>),
 * the previous tile staged in LDS; then, when d_info is given, one small kernel that sums the flags.  d_balls: n_balls rm_ball
 * records on the device.  d_reused int32[n_kept], optional: 1 where the tile was copied, 0 where it was evaluated.  d_info,
 * optional: an rm_tiles_update_info.  n_balls == 0 copies every block that was kept before.  RM_E_INVALID -- ahead of
 * RM_E_NO_DEVICE, RM_E_NO_SCENE after it -- for the lattice as the sparse entries check it, n_kept or n_prev_kept outside
 * 0 .. n_blocks, n_balls outside 0 .. RM_TILES_UPDATE_MAX_BALLS, with n_kept > 0 a null d_list, d_tiles or d_prev_slot (and
 * a null d_prev_tiles with n_prev_kept > 0), null d_balls with n_balls > 0, d_list / d_prev_slot / d_reused not 4-byte or
 * d_tiles / d_prev_tiles / d_balls / d_info not 8-byte aligned, and d_tiles[0 .. n_kept) overlapping d_prev_tiles[0 ..
 * n_prev_kept): slots shift when the kept set changes, so there is no in-place form.  RM_E_UNSUPPORTED, last, for
 * expression-program scenes (forests, presets 5 .. 18): rm_scene_tiles_device with exact = 1 remains their route; no buffer is
 * touched.  n_kept == 0 is RM_OK: zero info.  The knobs `filter` and `length` apply as for rm_scene_tiles_device.  Not a
 * render entry.  rm_last_kernel: tiles_update_kernel<GEN>. */
#define RM_TILES_UPDATE_MAX_BALLS 65536
typedef struct rm_ball {   /* 24 bytes */
    float   center[3];
    int32_t reserved;    /* 0 */
    double  radius;
} rm_ball;
typedef struct rm_tiles_update_info {   /* 32 bytes */
    int64_t n_kept, n_reused, n_evaluated, reserved;
} rm_tiles_update_info;
RM_API int rm_scene_edit_balls(rm_ctx *ctx, const rm_sphere_edit *edits, int32_t n_edits, rm_ball *balls, int32_t cap, int32_t *n_balls);
RM_API int rm_scene_tiles_update_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_prev_slot, const void *d_prev_tiles,
                                        int64_t n_prev_kept, const void *d_balls, int32_t n_balls, const void *d_list, int64_t n_kept,
                                        void *d_tiles, void *d_reused, void *d_info, void *stream);

/* ---- measures: how much there is of the solid -- volume, centroid, second moments, crossings, index box ---------- */

typedef struct rm_measure {   /* 176 bytes, 8-byte aligned; every field is written */
    int64_t n_points;         /* nu * nv * nw */
    int64_t n_inside;         /* inside points */
    int64_t n_nonfinite;      /* points whose value is not finite (the sparse path: of kept blocks only) */
    int64_t sum1[3];          /* sum of i, of j, of k over the inside points */
    int64_t sum2[6];          /* sum of i i, j j, k k, i j, j k, k i over the inside points */
    int64_t crossings[3];     /* axis A: lattice edges p -> p + e_A, both ends in the lattice, whose ends differ in `inside` */
    int32_t lo[3], hi[3];     /* the index box of the inside points; n_inside == 0: lo = INT32_MAX, hi = -1 */
    int64_t n_blocks, n_kept; /* the sparse path only, else 0 */
    int64_t n_blocks_inside;  /* the sparse path only, else 0: dropped blocks with d - iso < 0 */
    int64_t reserved;         /* written 0 */
} rm_measure;

struct rm_measure_world {   /* 120 bytes: rm_measure in the lattice's world units.  A tag without a typedef: the entry that
                             * fills it has the same name, so it is spelled `struct rm_measure_world` in C and C++ alike */
    double cell_volume;         /* |det(du, dv, dw)| */
    double volume;              /* n_inside * cell_volume */
    double centroid[3];         /* the lattice's point formula at the mean index, unrounded binary64; NaN when n_inside == 0 */
    double second[6];           /* integral of (x - c)(x - c)^T dV over the inside cells: xx, yy, zz, xy, yz, zx; 0 when n_inside == 0 */
    double projected_area[3];   /* crossings[A] * |step_B x step_C|: the surface projected along index axis A, with multiplicity */
    double area_estimate;       /* 2/3 of the sum of the three: an isotropic estimate, NOT a bound */
};

/* The meshers say where the surface is; these entries say how much it encloses.  Everything measured is an INTEGER -- counts of
 * inside lattice points, sums of their indices and index products, counts of sign-changing lattice edges --, so the result does
 * not depend on the order of summation and is compared bit for bit with a numpy restatement (tests/measure_model.py), the
 * standard the meshers are held to.  The rule:
 *   inside    point (i, j, k) is inside iff value < iso, the mesher's rule unchanged: NaN is outside, equality is outside.
 *   record    rm_measure above.  A point stands for its cell-sized box around it: volume = n_inside cells, and so on.
 *   overflow  both device entries (and rm_scene_measure) return RM_E_UNSUPPORTED -- behind their RM_E_INVALID checks, ahead of
 *             RM_E_NO_DEVICE -- when n_points * (max(nu, nv, nw) - 1)^2 does not fit below 2^63; every sum then fits an int64.
 *             (A dense volume of at most 2^30 points always fits.)
 *
 * rm_measure_field_device: d_values binary64 or binary32 (value_type: RM_MESH_F64 / RM_MESH_F32) laid out by the lattice
 * (lattice->time is not used), d_measure an rm_measure on the device; asynchronous on `stream`; it needs no scene.  A persistent
 * grid sized from the device's compute units; a wave takes whole lattice rows, a lane the points i = lane, lane + 64, ..., each
 * with its +i, +j and +k neighbours; one partial record per workgroup in the context's scratch buffer (ordered as
 * rm_mesh_field_device's use of it), then one workgroup adds the partials: no atomics, nothing to initialise, re-entrant.
 * RM_E_INVALID -- ahead of RM_E_NO_DEVICE, in this order -- for everything rm_scene_field refuses about a lattice, more than
 * 2^30 points, null d_values when the lattice has points, null d_measure, a non-finite iso, a value_type outside the enum,
 * d_measure or binary64 values not 8-byte aligned (binary32 values: 4).  Counts of 1 on an axis are fine: a slice has no edges
 * along that axis, and its cross-section is n_inside.  A lattice with a zero count is RM_OK: zero sums and the empty box are
 * written.  rm_last_kernel: measure_field_kernel<double> or <float> (measure_final_kernel for a lattice without points).
 *
 * rm_measure_tiles_device: the same record from what rm_scene_blocks_device (with d_dist) and the tile entries leave.
 *   ownership  block (bx, by, bz) owns the lattice points 8 bx .. 8 bx + 7 per axis; the last block of an axis also owns point
 *              8 nb when that index is <= n - 1.  Every lattice point is owned by exactly one block; an edge belongs to the
 *              owner of its low end; every owned point and owned edge of a block lies inside that block's 9 x 9 x 9 tile.
 *   kept       a kept block's owned points and edges are counted from its tile values; tile points beyond the lattice are
 *              skipped by index, not by value.
 *   dropped    d_slot[b] < 0.  If d_dist[b] - iso < 0 all owned points are inside: n_inside, sum1, sum2 and the box take the
 *              closed-form sums over the owned index ranges and no edge crosses; otherwise the block contributes nothing.  A
 *              dropped block never contributes to n_nonfinite.
 *   GUARANTEE  whenever the exact field is `lipschitz`-Lipschitz and the tiles hold that same field (option `exact`), no point
 *              of a dropped block's tile lies on the other side of iso than its centre (the coarse pass's bound covers the
 *              tile), so the record equals rm_measure_field_device's over the dense volume of that field, field by field --
 *              the block fields apart, and n_nonfinite counts kept blocks only.
 * One 256-thread workgroup per kept block, the tile staged in LDS, up to three owned points per lane, local sums in 32 bits and
 * the block's base indices joined once per workgroup; one lane per block for the closed forms; the partials and the last
 * workgroup as above.  RM_E_INVALID for the lattice as the sparse entries check it, any count below 2 (the lattice must have
 * blocks on every axis: a slice goes through the dense entry), n_kept outside 0 .. n_blocks, null d_measure, d_slot or d_dist,
 * null d_list or d_tiles with n_kept > 0, a non-finite iso, d_slot / d_list not 4-byte or d_dist / d_tiles / d_measure not
 * 8-byte aligned; then the overflow refusal; RM_E_NO_DEVICE.  It needs no scene.  rm_last_kernel: measure_tiles_kernel
 * (measure_blocks_kernel when nothing is kept).
 *
 * rm_scene_measure: host-side and synchronous -- the coarse pass with distances, the tile pass UNDER THE EXACT FIELD whatever
 * option `exact` says (the coarse pass decides by the exact field, so the tiles must hold it too), then the measure, all in the
 * context's scratch buffer as rm_scene_mesh_sparse uses it; n_kept is read back once.  sparse_info may be NULL.  The checks of
 * the entries for its own arguments (no alignment is asked of `out`), the overflow refusal, RM_E_NO_DEVICE; RM_E_NO_SCENE last.
 * None of these is a render entry: they neither consume nor fire rm_render_attach_diagnostics and leave rm_scene_set_time's
 * value alone.
 *
 * rm_measure_world: host-only, no ctx; RM_E_INVALID for a null argument or a lattice rm_scene_field refuses.  binary64, one
 * operation at a time, no contraction, in this order (u, v, w: du, dv, dw widened; N = (double)n_inside; S = (double)sum1,
 * Q = (double)sum2):
 *   cell_volume     fabs((u0 * (v1 * w2 - v2 * w1) - u1 * (v0 * w2 - v2 * w0)) + u2 * (v0 * w1 - v1 * w0))
 *   volume          N * cell_volume
 *   centroid[c]     m[a] = S[a] / N (the quiet NaN 0x7FF8000000000000 when n_inside == 0);
 *                   (((double)origin[c] + m[0] * u[c]) + m[1] * v[c]) + m[2] * w[c]
 *   second          the index covariance C[a][b] = Q[ab] - (S[a] * S[b]) / N (symmetric; ab as in sum2), pushed through
 *                   M = (u v w), M[p][a] the component p of step a: for (p, q) = xx, yy, zz, xy, yz, zx
 *                     t[a] = (C[a][0] * M[q][0] + C[a][1] * M[q][1]) + C[a][2] * M[q][2]
 *                     (((M[p][0] * t[0] + M[p][1] * t[1]) + M[p][2] * t[2]) * cell_volume)
 *                       + ((N * cell_volume) / 12.0) * ((M[p][0] * M[q][0] + M[p][1] * M[q][1]) + M[p][2] * M[q][2])
 *                   -- the second term is each cell's own box, u u^T + v v^T + w w^T over 12.  All 0.0 when n_inside == 0.
 *   projected_area  (double)crossings[A] * sqrt((x * x + y * y) + z * z), (x, y, z) = step_B x step_C =
 *                   (b1 * c2 - b2 * c1, b2 * c0 - b0 * c2, b0 * c1 - b1 * c0), (B, C) the other two axes in cyclic order.
 *                   It equals the integral of |n . a| dS over the staircase surface, with multiplicity.
 *   area_estimate   (2.0 / 3.0) * ((p[0] + p[1]) + p[2]).  An isotropic (Cauchy-Crofton) estimate, not a bound: exact in the
 *                   limit for a sphere, and off by factors between 2/3 and 2/sqrt(3) for flat faces (2/3 for an axis-aligned
 *                   one).  For a true area sum the mesh's quads.
 * For a slice (nw = 1) pass a unit dw orthogonal to du and dv to read `volume` as an area.
 * Out of scope: fractional (sub-cell) coverage, a true surface-area integral, and the N-API addon. */
RM_API int rm_measure_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso,
                                   void *d_measure, void *stream);
RM_API int rm_measure_tiles_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_slot, const void *d_list, int64_t n_kept,
                                   const void *d_dist, const void *d_tiles, double iso, void *d_measure, void *stream);
RM_API int rm_scene_measure(rm_ctx *ctx, const rm_lattice *lattice, double iso, double lipschitz, rm_measure *out,
                            rm_sparse_info *sparse_info);
RM_API int rm_measure_world(const rm_lattice *lattice, const rm_measure *measure, struct rm_measure_world *out);

/* ---- parts: the connected pieces of the solid (or of what surrounds it), numbered, with a measure each --------------- */

enum { RM_PARTS_INSIDE = 0, RM_PARTS_OUTSIDE = 1 };

typedef struct rm_parts_info {   /* 32 bytes, 8-byte aligned; every field is written */
    int64_t n_points;            /* nu * nv * nw */
    int64_t n_set;               /* points of the set S */
    int64_t n_parts;             /* connected components of S */
    int64_t gave_up;             /* non-zero: a thread ran out of its hop budget (below); labels and counts are then unspecified */
} rm_parts_info;

/* The measures are sums over the whole inside set; these entries split the set into its pieces.  Everything is an integer with
 * one right answer and is compared bit for bit with a numpy restatement (tests/parts_model.py).  The rule:
 *   set S      side = RM_PARTS_INSIDE: point (i, j, k) is in S iff value < iso -- the meshers' and the measures' rule unchanged:
 *              NaN is outside, equality is outside.  side = RM_PARTS_OUTSIDE: S is the complement, !(value < iso), NaN included.
 *   adjacency  two points of S are adjacent iff a lattice edge joins them (the 6-neighbourhood; the edges `crossings` counts).
 *              BOTH sides use this rule: the outside is 6-connected too, which is not the topologically dual choice (with a
 *              6-connected inside the dual outside would be 26-connected), so two outside pockets that touch across a diagonal
 *              count as two.
 *   part       a connected component of S.
 *   numbering  parts are numbered 0 .. n_parts - 1 in ascending order of their smallest linear index l = i + nu * (j + nv * k)
 *              (the numbering of scipy.ndimage.label(...)[0] - 1 on the [nw, nv, nu] array).
 *   labels     int32[n_points] in the lattice's order: the part's number, or -1 where the point is not in S.
 *   info       rm_parts_info above.
 *   records    part p < n_records gets an rm_measure, the struct unchanged: n_points is the lattice's; n_inside, sum1, sum2, lo
 *              and hi are taken over the part's points; crossings[A] counts the lattice edges along A with exactly one end in
 *              S, for the part of the end that is in S (two different parts are never adjacent, so every such edge belongs to
 *              one part); n_nonfinite, the block fields and reserved are 0.  Records p >= n_parts are the empty record (zero
 *              sums, lo = INT32_MAX, hi = -1); parts numbered >= n_records are skipped.  Hence, with side = RM_PARTS_INSIDE and
 *              n_records >= n_parts, the records summed field by field (the boxes united) equal rm_measure_field_device's
 *              record of the same values in n_inside, sum1, sum2, crossings, lo and hi.  A part touches the lattice's border
 *              iff its box does: an enclosed void is an outside part whose box does not, and needs no field of its own.
 *
 * rm_label_field_device: d_values as rm_measure_field_device takes them (it needs no scene; lattice->time is not used),
 * d_labels n_points int32 and d_info an rm_parts_info on the device; asynchronous on `stream`, re-entrant, nothing to
 * initialise.  d_labels is the parent array of a lock-free union-find: every point of S first points at the start of its run
 * along i within its wave and row (one ballot), unions with the -j and -k neighbours (and -i where a wave cut a run) link the
 * larger root below the smaller by atomicMin, so a part's root is its smallest index in whatever order the atomics arrive; the
 * roots are counted per workgroup, scanned, numbered by ballot rank into a map in the context's scratch buffer (ordered as
 * rm_mesh_field_device's use of it) and the labels rewritten through the map.  No thread waits for another; every loop lowers
 * an index at every step and has a budget of n_points steps, after which the thread stops and sets gave_up -- which no
 * well-formed run does.  RM_E_INVALID -- ahead of RM_E_NO_DEVICE -- for everything rm_measure_field_device refuses about the
 * lattice, the values, iso and value_type (more than 2^30 points among it), a `side` outside the enum, null d_labels when the
 * lattice has points, null d_info, d_labels not 4-byte or d_info not 8-byte aligned.  Counts of 1 on an axis are fine.  A lattice
 * with a zero count is RM_OK: info {0, 0, 0, 0}.  rm_last_kernel: parts_relabel_kernel (unchanged for a lattice without points).
 *
 * rm_measure_labels_device: the records from labels of that form alone -- the values are not needed; labels outside
 * -1 .. n_records - 1 are skipped.  d_records: n_records rm_measure on the device, all of them initialised by the entry.  A
 * persistent grid of waves over contiguous spans of the lattice; where a wave sees one label it keeps the sums in registers and
 * adds them to the record once, else once per run of a label along i; 64-bit integer atomicAdd and 32-bit atomicMin / atomicMax,
 * so the record does not depend on the order.  It uses no scratch.  RM_E_INVALID for the lattice, more than 2^30 points, null
 * d_labels when the lattice has points, n_records < 0 or > 2^20, null d_records with n_records > 0, d_labels not 4-byte or
 * d_records not 8-byte aligned; then the measures' overflow refusal RM_E_UNSUPPORTED; RM_E_NO_DEVICE.  rm_last_kernel:
 * parts_measure_kernel (parts_records_kernel for a lattice without points; unchanged with n_records = 0).
 *
 * rm_scene_parts: host-side and synchronous -- the dense volume of the active scene UNDER THE EXACT FIELD whatever option
 * `exact` says (as rm_scene_measure), the labels and the records, all in the context's scratch buffer, then one copy back.
 * labels_out may be NULL.  The checks of the two entries for its own arguments (no alignment is asked of host buffers), the
 * overflow refusal, RM_E_NO_DEVICE; RM_E_NO_SCENE last.  Not a render entry: it neither consumes nor fires
 * rm_render_attach_diagnostics and leaves rm_scene_set_time's value alone.
 * Out of scope: a sparse (tile) path -- dropped inside blocks would need a labelling rule of their own --, and the N-API addon. */
RM_API int rm_label_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso,
                                 int32_t side, void *d_labels, void *d_info, void *stream);
RM_API int rm_measure_labels_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_labels, int64_t n_records, void *d_records,
                                    void *stream);
RM_API int rm_scene_parts(rm_ctx *ctx, const rm_lattice *lattice, double iso, int32_t side, int32_t *labels_out, int64_t n_records,
                          rm_measure *records_out, rm_parts_info *info_out);

/* ---- distances: how far inside the solid (or outside it) every lattice point lies, exactly ------------------------------ */

#define RM_EDT_FAR INT32_MAX
typedef struct rm_edt_info {   /* 32 bytes, 8-byte aligned; every field is written */
    int64_t n_points;          /* nu * nv * nw */
    int64_t n_set;             /* points of the set S */
    int64_t max_d2;            /* the largest d2 over S; 0 when S is empty */
    int64_t argmax;            /* the smallest linear index of a point of S that attains it; -1 when S is empty */
} rm_edt_info;

/* The meshers, the measures and the parts ask on which side of iso a point lies; these entries say how far from the other
 * side it is.  The scene's own fields cannot: the exact field, a minimum over primitives, is exact outside a union and too
 * small inside it, the operator scenes hold bounds, and a caller's volume holds any values.  The answer here is the exact
 * Euclidean distance transform of the set on the lattice itself, in integers with one right answer, compared bit for bit with
 * a numpy restatement (tests/edt_model.py) and, as sqrt(d2), with scipy.ndimage.distance_transform_edt.  The rule:
 *   set S   exactly the parts' rule with the parts' `side` enum: RM_PARTS_INSIDE is value < iso (NaN is outside, equality is
 *           outside), RM_PARTS_OUTSIDE the complement, NaN included.  T is the complement of S WITHIN THE LATTICE: points
 *           beyond the lattice do not exist, they are neither S nor T (scipy's convention).  A solid that touches the border
 *           is therefore not cut there -- its points at the border are as deep as the nearest lattice point of T says --, so
 *           a lattice meant to measure thickness leaves a margin around the solid (Context.edt_box does).
 *   d2      int32[n_points] in the lattice's order: 0 where the point is not in S; where it is, the minimum over the points
 *           (i', j', k') of T of (i-i')^2 + (j-j')^2 + (k-k')^2.  Where T is empty d2 is RM_EDT_FAR at every point, and
 *           max_d2 is then RM_EDT_FAR (argmax 0).  These are INDEX units: the entries never read the lattice's steps;
 *           rm_lattice_cubic says whether, and by which factor, sqrt(d2) is a world distance.
 *   range   RM_E_UNSUPPORTED when (nu-1)^2 + (nv-1)^2 + (nw-1)^2 > INT32_MAX - 1, so every finite d2 lies below
 *           RM_EDT_FAR: a cube of 2^30 points is far inside the limit, a row of 46 341 points is the longest line allowed.
 *   info    rm_edt_info above.
 *
 * rm_edt_field_device: d_values as rm_label_field_device takes them (it needs no scene; lattice->time is not used), d_d2
 * n_points int32 and d_info an rm_edt_info on the device; asynchronous on `stream`, re-entrant, nothing to initialise.  The
 * squared distance separates by axis, so there are three passes over the resident volume, all in 32-bit integers.  Along i,
 * membership is one wave ballot and the nearest point of T on either side comes from bit scans of it (a row longer than a
 * wave walks on through the row's further 64-point segments).  Along j and then along k, one lane per line -- adjacent lanes
 * adjacent in i -- builds the lower envelope of the line's parabolas by Meijster's two scans, in place; the break point of two
 * parabolas is a floor division, RM_EDT_FAR marks an absent parabola and is never an addend, and no intermediate exceeds 32
 * bits.  An axis with one point has no pass: a slice gets the 2-D transform.  A line's envelope is a stack of (position, break
 * point, value) entries in the context's scratch buffer, laid out like the volume: 8 bytes per lattice point, plus 16 KiB of
 * partial maxima; max_d2, argmax and n_set are reduced per workgroup and then by one workgroup, without atomics, so nothing
 * depends on an order.  No thread waits for another and every loop is bounded by the length of its row or line: there is no
 * give-up flag.  RM_E_INVALID -- ahead of everything else -- for everything rm_label_field_device refuses about the lattice,
 * the values, value_type, iso and side (more than 2^30 points among it), null d_d2 when the lattice has points, null d_info,
 * d_d2 not 4-byte or d_info not 8-byte aligned; then the range refusal RM_E_UNSUPPORTED; then RM_E_NO_DEVICE.  Counts of 1 on
 * an axis are fine.  A lattice with a zero count is RM_OK: info {0, 0, 0, -1}.  rm_last_kernel: edt_axis_kernel (edt_rows_kernel
 * for a lattice that is a single row, which has no axis pass; unchanged for a lattice without points).
 *
 * rm_scene_edt: host-side and synchronous -- the dense volume of the active scene UNDER THE EXACT FIELD whatever option
 * `exact` says (as rm_scene_parts), the transform and its scratch, all in the context's scratch buffer, then one copy back.
 * d2_out may be NULL.  The same checks for its own arguments (no alignment is asked of host buffers), the range refusal,
 * RM_E_NO_DEVICE; RM_E_NO_SCENE last.  Not a render entry: it neither consumes nor fires rm_render_attach_diagnostics and
 * leaves rm_scene_set_time's value alone.
 *
 * rm_lattice_cubic: host-only, no ctx -- whether index distances are world distances up to one factor, and the factor.  All
 * arithmetic is binary64 of the widened components, one operation at a time; the length of a step is
 * sqrt((x*x + y*y) + z*z).  Only axes whose count exceeds 1 take part.  *step is the length of the first such axis's step (1.0
 * when there is none).  RM_OK when every other participating length differs from *step by at most 1e-5 * step and every
 * pairwise dot product of participating steps is at most 1e-5 * step^2 in magnitude; else RM_E_UNSUPPORTED with *step
 * untouched.  RM_E_INVALID for a null argument or a lattice rm_scene_field refuses.  Why 1e-5: the binary32 rounding of a
 * rotated cubic lattice's steps perturbs lengths and dot products by a few 1e-7 relative; 1e-5 leaves an order of magnitude
 * above that and still bounds the error of a world distance far below the half-cell quantisation of the transform itself.
 * Out of scope: the nearest point itself (a feature transform), world-metric transforms on non-cubic lattices, a sparse
 * (tile) path, sub-cell (fractional) distances, local thickness in the Hildebrand-Ruegsegger sense, and the N-API addon. */
RM_API int rm_edt_field_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso,
                               int32_t side, void *d_d2, void *d_info, void *stream);
RM_API int rm_scene_edt(rm_ctx *ctx, const rm_lattice *lattice, double iso, int32_t side, int32_t *d2_out, rm_edt_info *info_out);
RM_API int rm_lattice_cubic(const rm_lattice *lattice, double *step);

/* ---- sharp meshes: vertices from Hermite data (dual contouring's vertex rule) --------------------------------- */

typedef struct rm_sharp_query {  /* 32 bytes */
    double  iso;        /* the surface is D == iso; finite */
    double  rank_tol;   /* an eigenvalue counts when it exceeds rank_tol * the largest; in [0, 1] */
    double  reach;      /* a vertex may lie up to reach * rho from its cell's centre; finite, >= 0 */
    int32_t refine;     /* R, 0 .. 8: refinements of each crossing's bracket */
    int32_t reserved;   /* 0 */
} rm_sharp_query;

/* Surface nets place a vertex at the mean of its cell's edge crossings, which cannot represent a crease: every edge of a box
 * comes out chamfered and every corner cut off by about half a cell, and the snap of rm_scene_points moves a vertex onto ONE
 * face, not onto the line where two meet.  This pass keeps the topology -- one vertex per active cell, the quads untouched --
 * and moves each vertex to the point that minimises the distance to the tangent planes sampled at its cell's edge crossings (the
 * Hermite data), as dual contouring does.  The rule, operation for operation (tests/sharp_model.py restates it; results are
 * equal byte for byte).  All arithmetic is binary64, one operation at a time, no contraction, in the stated order.
 *   input     an rm_lattice (as rm_scene_field takes and checks it), the key l = (k * nv + j) * nu + i of the vertex's cell (what
 *             rm_mesh_cells_device and the sparse mesher's `cells` return) and the query.  D is Scene.getDistance with
 *             Scene.updateTime(lattice->time), exactly as rm_scene_distance returns it -- with option `exact` the exact field E,
 *             as for the point queries; the primitive count of every evaluation made is added to count.
 *   corners   the eight corner values are D at the lattice's own points (i + dx, j + dy, k + dz); inside and active follow
 *             rm_mesh_field_device's rule (a hole is not active).  A key that names no cell (l < 0, l >= nu * nv * nw, or an
 *             index at the last point of its axis): position (0, 0, 0), feature -1, count 0, nothing is evaluated.  A cell that
 *             is not active: position = the lattice's point rule at index (i + 0.5, j + 0.5, k + 0.5), feature -1, count = the
 *             corners' counts, nothing more is evaluated.
 *   crossings the twelve edges in the surface-nets order, a and b the values at an edge's low and high end.  When exactly one end
 *             is inside: start the bracket at (tl, fl, th, fh) = (0, a, 1, b) and repeat R times
 *                 t = tl + (iso - fl) * (th - tl) / (fh - fl)                  (product, quotient, sum)
 *                 f = D(P(t))         P(t): the point rule with index (double)index + t on the edge's axis, one rounding
 *                 if (f < iso) == (a < iso): (tl, fl) = (t, f)   else: (th, fh) = (t, f)
 *             then form t once more from the final bracket: p = P(t), d = D(p), n = G(p, d), G exactly rm_scene_points' G, its
 *             three evaluations counted.  A t or a component of P(t) that is not finite drops the crossing at once, before
 *             anything is evaluated there; a non-finite component of n drops it too.
 *   quadric   over the kept crossings in edge order, p and n widened: m = (sum of p) / (double)kept per component;
 *             A = sum of n n^T as six sums a00, a01, a02, a11, a12, a22; b = sum of n * s with
 *             s = (n.x * (p.x - m.x) + n.y * (p.y - m.y)) + n.z * (p.z - m.z).  No kept crossing: position as for a cell that is
 *             not active, feature 0.
 *   eigen     six cyclic Jacobi sweeps over (p, q) = (0, 1), (0, 2), (1, 2), V = I at the start.  a[p][q] == 0 skips the
 *             rotation; else theta = (aqq - app) / (2 * apq); t = 1 / (|theta| + sqrt(theta * theta + 1)), negated unless
 *             theta >= 0; c = 1 / sqrt(t * t + 1); s = t * c; h = t * apq; app = app - h; aqq = aqq + h; apq = 0; with r the
 *             third index (arp, arq) = (c * arp - s * arq, s * arp + c * arq), kept symmetric; every row k of V likewise:
 *             (V[k][p], V[k][q]) = (c * V[k][p] - s * V[k][q], s * V[k][p] + c * V[k][q]).  Eigenvalue i is a[i][i], its vector
 *             column i of V.  The pairs are put in descending order by compare-and-swap on positions (0, 1), (1, 2), (0, 1),
 *             swapping only when the later value is strictly greater: on ties the lower index comes first.
 *   rank      lmax is the first eigenvalue; r0 = the number of eigenvalues > rank_tol * lmax, 0 unless lmax > 0.  c is the
 *             unrounded binary64 cell centre (index + 0.5); rho is half the longest of |(du + dv) + dw|, |(du + dv) - dw|,
 *             |(du - dv) + dw|, |(du - dv) - dw|, each norm sqrt((x * x + y * y) + z * z); limit = reach * rho.  With
 *             k_i = ((v_i.x * b.x + v_i.y * b.y) + v_i.z * b.z) / lambda_i, for r = r0 down to 1:
 *             x = ((m + v_0 * k_0) + v_1 * k_1) + v_2 * k_2 per component, the first r terms only; x is accepted when
 *             sqrt((dx * dx + dy * dy) + dz * dz) <= limit for (dx, dy, dz) = x - c.  None accepted: x = m, r = 0.
 *   outputs   position = f32(x); feature = r: 1 a face, 2 an edge, 3 a corner, 0 the mean of the crossings; count exact u32.
 * Known limit: a cell that an edge of the solid clips without crossing one of the cell's own lattice edges sees one face
 * only (rank 1) and stays where that face puts it; that is inherent to the method.  About R + 4 evaluations per crossing and
 * 8 per cell: some 32 per vertex with R = 2.
 *
 * rm_mesh_cells_device: the key of every vertex of rm_mesh_field_device's mesh of the same values, d_cells int64[cap_vertices],
 * by the same count and scan (three kernels).  Checks, the counting call (capacity 0, null buffer) and the truncation protocol
 * are rm_mesh_field_device's, with d_cells 8-byte aligned; d_info receives the same rm_mesh_info.
 *
 * rm_scene_sharpen_device: n vertices, one launch, asynchronous on `stream`.  d_cells int64[n], d_position f32[3n], d_feature
 * i32[n] or NULL, d_count u32[n] or NULL.  RM_E_INVALID -- ahead of RM_E_NO_DEVICE and RM_E_NO_SCENE -- for a lattice
 * rm_scene_field refuses, a null query, a non-zero reserved, R outside 0 .. 8, a non-finite iso, a rank_tol outside [0, 1], a
 * reach that is not finite or < 0, n < 0 or n > INT32_MAX, null cells or position with n > 0, cells not 8-byte or another
 * buffer not 4-byte aligned.  n == 0 is RM_OK.  Keys may repeat and come in any order; consecutive keys of neighbouring cells
 * keep a workgroup's tree walks coherent.  Not a render entry: it neither consumes nor fires rm_render_attach_diagnostics and
 * leaves rm_scene_set_time's value alone; knobs apply as for rm_scene_field (`filter`, `length`, `exact`); ahead-of-time
 * kernels only.  rm_last_kernel names the sharp_kernel<ACCEL, GEN> instantiation.
 * rm_scene_sharpen: host buffers, synchronous, chunked through the context's scratch buffer by 4 M vertices. */
RM_API int rm_mesh_cells_device(rm_ctx *ctx, const rm_lattice *lattice, const void *d_values, int32_t value_type, double iso,
                                void *d_cells, int64_t cap_vertices, void *d_info, void *stream);
RM_API int rm_scene_sharpen_device(rm_ctx *ctx, const rm_lattice *lattice, const rm_sharp_query *q, int64_t n, const void *d_cells,
                                   void *d_position, void *d_feature, void *d_count, void *stream);
RM_API int rm_scene_sharpen(rm_ctx *ctx, const rm_lattice *lattice, const rm_sharp_query *q, int64_t n, const int64_t *cells,
                            float *position, int32_t *feature, uint32_t *count);

/* ---- ray queries ------------------------------------------------------------------ */

typedef struct rm_ray_query {
    int32_t algorithm;        /* rm_algorithm; unknown -> sphere tracer (raymarchWorker.ts:49-68)          */
    int32_t normal;           /* 1: getNormal at hits, its 4 evaluations counted (raymarcher.ts:94-102)     */
    double  time;             /* Scene.updateTime (AnimatedTranslate) for this query; rm_scene_set_time's value is kept */
    double  overshoot_factor; /* NaN = JS undefined -> 1.2 */
    double  step_size;        /* NaN = JS undefined -> 0.1 */
} rm_ray_query;

/* Raymarcher.rayMarch (+ getNormal) for n caller-supplied rays through the ACTIVE scene (as rm_scene_distance), host
 * buffers (synchronous).  The marchers of sphereTracer.ts:15-83, fixedStep.ts:21-94, adaptiveStep.ts:22-105,
 * adaptiveStepV2.ts:22-124 and adaptiveStepV3.ts:22-137 with the scene's acceleration structure (BVH.onRayMarchStart /
 * onRayMarchStep, bvh.ts:181-240; Octree.marchRay, octree.ts:250-294), exactly as a render marches its camera rays, for
 * ray i = (origins_xyz[3i..3i+2], dirs_xyz[3i..3i+2]) as Float32Array vec3s.  The direction is used as given: rayMarch
 * does not normalise it.  Per ray: t[i] = the value rayMarch returns (>= 10 = miss for the sphere tracer; FixedStep /
 * AdaptiveStep return 10 unless they hit), iters[i] and sdf_calls[i] = the iteration and Scene.getDistance primitive
 * counts, exact (the reference's Uint16Array buffers hold them mod 65536; with q->normal, sdf_calls includes getNormal's
 * four evaluations), normal_xyz[3i..3i+2] = the normalised binary32 getNormal result at hitPosition = f32(o + d t)
 * (raymarcher.ts:94-102,123-135), (0, 0, 0) for t >= 10 or without q->normal.  Every output may be NULL.
 * RM_E_NO_DEVICE for a host-only context, RM_E_NO_SCENE before any scene, RM_E_INVALID for a null query, n < 0,
 * n > INT32_MAX, null ray buffers with n > 0 or a non-finite origin or direction component; n == 0 is RM_OK.
 * Knobs (rm_set_option) apply as for the one-ray-per-lane render and never change results; `length` selects the
 * vec3.length form.  Scenes whose renders run a run-time specialised kernel are marched by the ahead-of-time kernels
 * here (same values).  A ray query is not a render call: it neither consumes nor fires rm_render_attach_diagnostics.
 * rm_last_kernel names the cast_kernel<...> instantiation.  Large batches go through the context's scratch buffer in
 * chunks of 4 M rays. */
RM_API int rm_ray_march(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const float *origins_xyz, const float *dirs_xyz,
                        double *t, uint32_t *iters, uint32_t *sdf_calls, float *normal_xyz);

/* Same with device pointers (origins, dirs f32[3n]; t f64[n]; iters, sdf_calls u32[n]; normal f32[3n]; each output may be
 * NULL), asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream).  Non-finite input is the
 * caller's responsibility: it is not checked, and every march loop still ends (they are bounded). */
RM_API int rm_ray_march_device(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *d_origins, const void *d_dirs,
                               void *d_t, void *d_iters, void *d_sdf_calls, void *d_normal, void *stream);

/* The rays runRaymarcher casts for rows [y_start, y_end) of a W x H frame (raymarcher.ts:61-88), host-only, no ctx:
 * origin3 = the camera position (Camera.setAngles(pitch, yaw) + getPosition, camera.ts:58-69,81-88),
 * dirs_xyz[3 * (local_row * W + x)] = the binary32 direction after vec3.fromValues(u, v, -1), transformMat3 and
 * normalize.  Marched with rm_ray_march they give the pixels of that frame.  RM_E_INVALID unless W >= 0, H > 0,
 * 0 <= y_start <= y_end <= H and the angles are finite. */
RM_API int rm_camera_rays(int32_t width, int32_t height, double pitch, double yaw, int32_t y_start, int32_t y_end,
                          float *origin3, float *dirs_xyz);

/* ---- picking and read-back of a scene's objects ------------------------------------- */

/* rm_ray_march plus the object each ray hit: the same arguments, the same checks and return codes, and t, iters,
 * sdf_calls, normal_xyz bit-identical to what rm_ray_march returns for the same rays and query.  object[i] is an index
 * into the scene's objects (Scene.objectSDFs, scene.ts:16,43) in the order the scene was built in: the order of
 * sceneManager.ts for a preset, the array index for rm_scene_from_spheres / rm_scene_from_prims, the index into roots[]
 * for rm_scene_from_nodes -- never a device slot (a BVH stores a sphere list in leaf order).  The rule:
 *   - t[i] >= 10 (getMaxDistance, the rule raymarcher.ts:98 skips the normal by): -1, nothing is evaluated;
 *   - else p = hitPosition = f32(o + d t) (vec3.scaleAndAdd, raymarcher.ts:94-95; getNormal's point) and
 *     D = Scene.getDistance(p).  The candidates are exactly the objects getDistance evaluates at p (scene.ts:144-190):
 *     Octree: the primitives of the leaf findNode(p) returns (none for an empty leaf; every object outside the cube);
 *     BVH: getPrimitivesAt(p), every object when that set is empty (scene.ts:173); None: every object.  object[i] is the
 *     lowest index among the candidates whose primitive.sdf(p) == D (IEEE ==); when D is NaN, the lowest-index candidate
 *     whose sdf is NaN; -1 when no candidate matches (D from an empty octree leaf's minDistance * 0.99, or the start
 *     value 10).
 * The pick is no part of the reference's work: it adds nothing to sdf_calls.  Every output may be NULL.  A pick neither
 * consumes nor fires rm_render_attach_diagnostics and leaves rm_scene_set_time's value alone; rm_last_kernel names the
 * pick_kernel<...> instantiation.  Host buffers, synchronous, chunked through the context's scratch buffer. */
RM_API int rm_ray_pick(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const float *origins_xyz, const float *dirs_xyz,
                       double *t, uint32_t *iters, uint32_t *sdf_calls, float *normal_xyz, int32_t *object);

/* Same with device pointers (object: i32[n]), asynchronous on `stream`, as rm_ray_march_device. */
RM_API int rm_ray_pick_device(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *d_origins, const void *d_dirs,
                              void *d_t, void *d_iters, void *d_sdf_calls, void *d_normal, void *d_object, void *stream);

/* ---- light queries: shadow rays and ambient occlusion at hits ------------------------ */

typedef struct rm_light {
    float   dir[3];        /* towards the light, used as given (not normalised), like a ray direction */
    int32_t ao_samples;    /* K, 0 .. 8; 0: no occlusion samples, ao = 1 */
    double  bias;          /* shadow-ray origin offset along the normal, finite, >= 0 */
    double  ao_step;       /* spacing of the occlusion samples, finite, > 0 when K > 0 */
    double  ao_strength;   /* finite, >= 0 */
} rm_light;

/* rm_ray_march with q->normal = 1, plus two light terms at each hit, in ONE launch: a shadow ray towards a directional light
 * through the query's own marcher and the scene's acceleration structure, and K ambient-occlusion samples of
 * Scene.getDistance along the normal.  q->normal is ignored: normals are always computed and their four evaluations
 * counted in sdf_calls.  The reference has neither term (its PhongModel has a light direction and no shadows); both are
 * built from its own functions only.  The rule, per ray (o, d):
 *   1. t, iters, sdf_calls, normal_xyz are bit-identical to rm_ray_march with q->normal = 1 for the same ray and query.
 *   2. t >= 10 (getMaxDistance) or a normal of (0, 0, 0) (zero gradient): lit = 1, ao = 1, iters2 = 0, sdf_calls2 = 0;
 *      nothing further is evaluated.
 *   3. Else p = hitPosition = f32(o + d t) (vec3.scaleAndAdd, raymarcher.ts:94-95; getNormal's point), n = the binary32
 *      normal, L = light->dir.
 *   4. c = (double)n0 L0 + (double)n1 L1 + (double)n2 L2, left to right in binary64, no contraction.  c <= 0 or NaN:
 *      lit = 0, no shadow ray (iters2 = 0, sdf_calls2 starts at 0).  Else the shadow origin is s = f32(p + n bias) per
 *      component (the same scaleAndAdd form), and the ray (s, L) is marched by q's marcher with q's time, overshoot and
 *      step through the acceleration structure: exactly what rm_ray_march returns for that ray with q->normal = 0.
 *      lit = (t_s >= 10) ? 1 : 0, iters2 = its iterations, sdf_calls2 starts as its SDF calls.
 *   5. For k = 1 .. K: h_k = k ao_step, q_k = f32(p + n h_k), d_k = Scene.getDistance(q_k) at q's time, its primitive
 *      count added to sdf_calls2; occ = sum of (h_k - d_k) 2^(1-k) in order of increasing k in binary64;
 *      x = 1 - ao_strength occ; ao = (float)(x > 0 ? (x > 1 ? 1 : x) : 0), so NaN gives 0.  K = 0: ao = 1.
 *      getDistance is taken as it is (scene.ts:144-190): an empty octree leaf answers minDistance * 0.99, the minimum
 *      starts at 10, and a point in no BVH leaf box is measured against every primitive -- d_k is a bound the marchers
 *      are satisfied with, not always the exact distance, and the occlusion term inherits that.
 * lit, ao: f32[n]; iters2, sdf_calls2: u32[n]; every output may be NULL.  Checks and return codes are rm_ray_march's,
 * plus RM_E_INVALID -- like every argument check ahead of RM_E_NO_DEVICE and RM_E_NO_SCENE -- for a null light, a
 * non-finite dir component, ao_samples outside 0 .. 8, a non-finite or negative bias or ao_strength, a non-finite
 * ao_step or one that is not positive when K > 0; n == 0 is RM_OK.  A bias at or below the marchers' hit threshold
 * (0.001) makes every shadow ray hit its own surface at once.  Not a render entry: it neither consumes nor fires
 * rm_render_attach_diagnostics and leaves rm_scene_set_time's value alone; rm_last_kernel names the light_kernel<...>
 * instantiation.  Lanes whose ray missed idle while their wave's hits run the secondary phases.  Host buffers,
 * synchronous, chunked through the context's scratch buffer as rm_ray_march. */
RM_API int rm_ray_light(rm_ctx *ctx, const rm_ray_query *q, const rm_light *light, int64_t n, const float *origins_xyz,
                        const float *dirs_xyz, double *t, uint32_t *iters, uint32_t *sdf_calls, float *normal_xyz,
                        float *lit, float *ao, uint32_t *iters2, uint32_t *sdf_calls2);

/* Same with device pointers, asynchronous on `stream`, as rm_ray_march_device. */
RM_API int rm_ray_light_device(rm_ctx *ctx, const rm_ray_query *q, const rm_light *light, int64_t n,
                               const void *d_origins, const void *d_dirs, void *d_t, void *d_iters, void *d_sdf_calls,
                               void *d_normal, void *d_lit, void *d_ao, void *d_iters2, void *d_sdf_calls2, void *stream);

/* ---- walk queries: how a marcher walked a ray ------------------------------------------ */

typedef enum rm_step_kind { RM_STEP_EVAL = 0, RM_STEP_SKIP = 1 } rm_step_kind;
typedef struct rm_step {      /* 24 bytes */
    double   t;               /* march parameter the record was made at */
    double   value;           /* EVAL: the distance returned; SKIP: the skip length (> 0) */
    uint32_t count;           /* EVAL: primitives that evaluation counted; SKIP: 0 */
    int32_t  kind;            /* rm_step_kind */
} rm_step;

typedef enum rm_walk_end { RM_END_HIT = 0, RM_END_FAR = 1, RM_END_STEPS = 2, RM_END_ACCEL = 3 } rm_walk_end;
typedef struct rm_walk {      /* 48 bytes */
    double   t;               /* what rm_ray_march returns for the ray */
    double   min_dist, t_min; /* smallest EVAL value and the t of the record that set it */
    double   skipped;         /* sum of the SKIP values */
    uint32_t evals, skips;    /* EVAL records (== iters) and SKIP records the walk produced */
    uint32_t sdf_calls;       /* sum of the EVAL counts (== rm_ray_march's sdf_calls with normal = 0) */
    int32_t  end;             /* rm_walk_end */
} rm_walk;

#define RM_WALK_MAX_STEPS 256

/* The walk itself, for n caller-supplied rays, in ONE launch: a summary per ray (walks[i]) and, with steps != NULL, the
 * ray's step trace, one record per distance evaluation and per acceleration-structure skip.  The ray is marched exactly
 * as rm_ray_march marches it with q->normal = 0; q->normal is ignored: a walk never evaluates a normal.  The rule, per
 * ray (o, d):
 *   EVAL  every call of Scene.getDistance the marcher makes -- the calls that add to iters, AdaptiveStepV3's bridging
 *         third evaluation (adaptiveStepV3.ts:103-130) included -- produces one EVAL record: t = the parameter the point
 *         p = f32(o + d t) was formed at, value = the distance, count = the primitives that call counted.
 *   SKIP  every loop trip in which the acceleration structure answered a positive skip (BVH.onRayMarchStep: tEnter - t,
 *         bvh.ts:204-240; Octree.marchRay's step, octree.ts:250-294) produces one SKIP record: t = the parameter before
 *         the skip, value = the skip, count = 0.  The marcher continues at t + value, one binary64 addition.
 *   No other record: V2's and V3's step-back moves t without one, and the next EVAL record's t shows it.  Records are in
 *   program order, and no walk produces more than 200 (100 or 200 loop trips; V3 evaluates at most twice in each of 100).
 *   end   the first of: RM_END_ACCEL -- the BVH gave no interval at onRayMarchStart or onRayMarchStep answered -1 (t is
 *         10, possibly with no record at all); RM_END_HIT -- an evaluation below 0.001 ended the loop; RM_END_FAR --
 *         t > 10 ended it, after a step or after a skip; RM_END_STEPS -- the trip limit ran out.  FixedStep and
 *         AdaptiveStep return t = 10 for FAR and STEPS, as rm_ray_march does.
 *   min_dist starts at +infinity and is replaced when value < min_dist (a NaN is never taken; the first record to reach
 *   the minimum keeps t_min); without an EVAL record min_dist is +infinity and t_min 0.  skipped starts at 0.0 and adds
 *   the skips in order, in binary64.  evals == rm_ray_march's iters and sdf_calls its sdf_calls, t its t.
 * walks[i] is always written whole.  With steps != NULL the first min(cap, evals + skips) records of ray i go to
 * steps[i * cap ...] and the remaining slots of that ray are left untouched; steps == NULL gives summaries only, and
 * walks may be NULL when steps is not.  Checks and return codes are rm_ray_march's, plus RM_E_INVALID -- like every
 * argument check ahead of RM_E_NO_DEVICE and RM_E_NO_SCENE -- for a cap outside 0 .. RM_WALK_MAX_STEPS, steps != NULL
 * with cap == 0, and both outputs NULL with n > 0; n == 0 is RM_OK.  Not a render entry: it neither consumes nor fires
 * rm_render_attach_diagnostics and leaves rm_scene_set_time's value alone; rm_last_kernel names the walk_kernel<...>
 * instantiation.  Host buffers, synchronous, chunked through the context's scratch buffer as rm_ray_march: 4 M rays a
 * chunk for summaries only; with step records at most 64 MiB of them a chunk and at least one ray (cap 256: 10 922 rays). */
RM_API int rm_ray_walk(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const float *origins_xyz, const float *dirs_xyz,
                       int32_t cap, rm_walk *walks, rm_step *steps);

/* Same with device pointers (d_walks: rm_walk[n]; d_steps: rm_step[n * cap]), asynchronous on `stream`, as
 * rm_ray_march_device.  Also RM_E_INVALID for a d_walks or d_steps that is not 8-byte aligned. */
RM_API int rm_ray_walk_device(rm_ctx *ctx, const rm_ray_query *q, int64_t n, const void *d_origins, const void *d_dirs,
                              int32_t cap, void *d_walks, void *d_steps, void *stream);

/* ---- point queries: distance, normal, object and projection onto the surface ------------- */

enum { RM_POINT_NORMAL = 1 };    /* rm_point_query.flags */

typedef struct rm_point_query {  /* 40 bytes */
    double  time;        /* Scene.updateTime for this query; rm_scene_set_time's value is kept */
    double  iso;         /* the surface is getDistance == iso; finite */
    double  snap_tol;    /* finite, >= 0 */
    int32_t snap_steps;  /* K, 0 .. 16; 0: the points as given */
    int32_t flags;       /* RM_POINT_NORMAL or 0 */
    int32_t reserved[2]; /* 0 */
} rm_point_query;

/* What can be asked about a point, for n caller-supplied points in ONE launch: Scene.getDistance, the normal getNormal
 * returns there, the object that attains the distance, and the point moved onto the surface getDistance == iso by up to K
 * steps along the normal -- for the vertices of a mesh, the hit points of a ray query, a 3D cursor, a collision probe.  The
 * reference has no such entry; everything is built from its own getDistance (scene.ts:144-190) and getNormal
 * (raymarcher.ts:123-135) only.  The rule, per point p0 (three binary32 values), with D(x) = Scene.getDistance(x) with
 * Scene.updateTime(q->time), exactly as rm_scene_distance returns it, its primitive count added to count:
 *     p = p0; steps = 0
 *     loop:  d = D(p)
 *            r = d - iso                                              (binary64)
 *            if steps == K or !(|r| > snap_tol): break                (a NaN r breaks)
 *            g = G(p, d);  if g == (0, 0, 0): break                   (IEEE ==: -0 is 0)
 *            p.c = f32((double)p.c + (double)g.c * (-r))              per component c: binary64, no contraction, ONE rounding
 *            steps += 1
 *   G(p, d) is getNormal at p with its first evaluation taken as d: q_c = p with component c replaced by
 *           f32((double)p.c - 0.01); n.c = f32(d - D(q_c)) for c = x, y, z in that order; len = n.x n.x + n.y n.y + n.z n.z in
 *           binary64, left to right; n.c = f32(n.c * (1 / sqrt(len))) when len > 0, f32(n.c * len) otherwise.  It is the
 *           arithmetic of the normal rm_ray_march returns, operation for operation; its three evaluations are counted.
 *   outputs are taken at the final p: position = p; dist = d, the un-offset getDistance, always D(position); steps as
 *           the loop left it; normal = G(p, d) with RM_POINT_NORMAL, else (0, 0, 0).  G is evaluated at most once per point
 *           visited: a loop that ended on the zero-gradient break has it already.  count is the primitives of every
 *           evaluation actually made, exact u32.
 *   object  follows rm_ray_pick's candidate rule at position with D = dist, without its t >= 10 clause: the candidates are
 *           what getDistance evaluates there, object is the lowest index whose Primitive.sdf equals D under IEEE ==, the
 *           lowest NaN candidate when D is NaN, -1 without a match.  It is computed only when the output is non-NULL and adds
 *           nothing to count.
 * getDistance is taken as it is: an empty octree leaf answers the constant minDistance * 0.99, so G is (0, 0, 0) there and a
 * projection stops at once with steps = 0, and under a BVH D over-estimates inside leaf boxes: a projection, a nearest-object
 * or a collision probe wants option `exact` (below), which puts the exact field E in D's place whatever the acceleration.  With
 * K = 0, no flags and exact = 0, dist and count are rm_scene_distance's.
 * position, normal: f32[3n]; dist: f64[n]; object, steps: i32[n]; count: u32[n]; every output may be NULL.  RM_E_INVALID --
 * like every argument check ahead of RM_E_NO_DEVICE and RM_E_NO_SCENE -- for a null query, a non-zero reserved, unknown flag
 * bits, K outside 0 .. 16, a non-finite time, iso or snap_tol, a negative snap_tol, n < 0 or n > INT32_MAX, null points with
 * n > 0, all six outputs NULL with n > 0, a dist that is not 8-byte or another buffer that is not 4-byte aligned, and a
 * non-finite point component.  n == 0 is RM_OK.  Not a render entry: it neither consumes nor fires
 * rm_render_attach_diagnostics and leaves rm_scene_set_time's value alone; knobs apply as for rm_scene_distance (`filter`,
 * `length`).  Scenes whose renders run a run-time specialised kernel are served by the ahead-of-time kernels here (same
 * values).  rm_last_kernel names the point_kernel<ACCEL, GEN> instantiation.  Lanes that converge early idle until their
 * wave's last lane has.  Host buffers, synchronous, chunked through the context's scratch buffer in chunks of 4 M points;
 * only the outputs asked for are staged and copied back. */
RM_API int rm_scene_points(rm_ctx *ctx, const rm_point_query *q, int64_t n, const float *points_xyz, float *position,
                           double *dist, float *normal, int32_t *object, int32_t *steps, uint32_t *count);

/* Same with device pointers, asynchronous on `stream`, as rm_ray_march_device: one launch.  The points are not checked
 * (every loop is bounded by K).  d_position may be d_points: a lane reads its point before it writes. */
RM_API int rm_scene_points_device(rm_ctx *ctx, const rm_point_query *q, int64_t n, const void *d_points, void *d_position,
                                  void *d_dist, void *d_normal, void *d_object, void *d_steps, void *d_count, void *stream);

/* The binary32 light direction PhongModel normalises from (1, -1, 1.5) (phongModel.ts:15-16), what RM_SHADE_PHONG and
 * rm_shade_lit shade with; host-only, no ctx.  RM_E_INVALID for a null pointer. */
RM_API int rm_phong_light(float dir3[3]);

/* Reads back object `index` of the active scene as an expression tree in the form rm_scene_from_nodes takes: operands
 * before their user, the object's root last.  A sphere, box or torus of a list scene is one leaf node (its world_to_local
 * and params; a sphere of rm_scene_from_spheres at rm_make_transform of its centre).  An uploaded scene comes back as it
 * was given, in upload order (never in a BVH's leaf order); a preset's objects come back as the reference holds them:
 * Box.halfSize, Repetition.spacing and AnimatedTranslate.direction as their binary32 values, operators with the
 * Primitive.transform their constructors derive (Round / Twist / Repetition / AnimatedTranslate: the operand's; the smooth
 * unions: identity).  Operand indices a node does not use are -1.  *n_nodes (may be NULL) always receives the node count;
 * the nodes are written only if cap >= that count, else nothing is (RM_OK either way).  RM_E_NO_SCENE before any scene,
 * RM_E_INVALID for an index out of range, cap < 0 or a null buffer with cap > 0.  Works on a host-only context. */
RM_API int rm_scene_object(rm_ctx *ctx, int32_t index, rm_node *nodes, int32_t cap, int32_t *n_nodes);

/* ---- render -------------------------------------------------------------------- */

/* Replaces the worker's onmessage (raymarchWorker.ts:33-92) = Raymarcher.runRaymarcher
 * (raymarcher.ts:46-109) for one row tile, host buffers (synchronous).  Counters are
 * (re)initialised per pixel (raymarcher.ts:79-80); buffers need no pre-clear. */
RM_API int rm_render_tile(rm_ctx *ctx, const rm_job *job, uint8_t *depth, uint8_t *normal,
                          uint16_t *sdf, uint16_t *iters);

/* Same with device pointers (hipMalloc / torch CUDA tensors), asynchronous on `stream`
 * (a hipStream_t passed as void*, NULL = default stream).  rgba may be NULL; when not,
 * ShadingModel.shade (shading_models/, all four) is fused behind the march.  depth, normal, sdf, iters may
 * each be NULL when the caller does not want that G-buffer (rgba then still sees them). */
RM_API int rm_render_tile_device(rm_ctx *ctx, const rm_job *job, int32_t shader, void *d_depth,
                                 void *d_normal, void *d_sdf, void *d_iters, void *d_rgba,
                                 void *stream);

/* ---- many frames of one scene in one launch ----------------------------------------- */

/* What one frame of rm_render_frames_device has of its own: Job.camera.pitch / .yaw and Job.time. */
typedef struct rm_view { double camera_pitch, camera_yaw, time; } rm_view;

/* n_views frames of ONE scene in ONE launch: a yaw sweep with its metric series (main.ts:438-441,550-566), an animated
 * scene over time, an orbit of thumbnails -- consumers of a sequence of small frames, which rendered one call at a time pay a
 * launch, a parameter block and a host round trip per frame and cannot fill the GPU (a 256 x 256 frame is 1 024 waves).
 *   job     everything the frames share -- width, height, rows [y_start, y_end), algorithm, scene / preset, acceleration
 *           structure, overshoot, step size -- defaulted, clamped and checked exactly as rm_render_tile_device does.  Its own
 *           camera_pitch, camera_yaw and time are ignored.
 *   views   host memory, copied: views[k] gives frame k its pitch (clamped per view, camera.ts:59), yaw and time.  The cameras
 *           are built on the host by the code behind rm_camera_from_angles.
 * Frame k is bit for bit what rm_render_tile_device writes for the same job with views[k]'s three fields; with
 * h = max(0, y_end - y_start) it occupies elements [k * W * h, (k + 1) * W * h) of each buffer (x3 normal, x4 rgba).  Each of
 * the five pixel buffers may be NULL; with d_rgba the shader is fused and still sees the G-buffers.
 *   d_acc   NULL, or n_views accumulators of 32 bytes (the layout of rm_reduce_counters_enqueue, 8-byte aligned): entry k
 *           receives what rm_render_attach_diagnostics would leave for frame k -- sum / max / min of the stored sdfEval values
 *           and the sum of the stored iteration values, Uint16Array wrap included -- written by the render launch itself (every
 *           frame has its own accumulator slots and completion count, the last wave of a frame writes its entry): no
 *           initialising launch, no second pass, no memset.  With all five pixel buffers NULL the call writes the metric
 *           series and nothing else.  Frames without a pixel (h == 0 or W == 0): the neutral elements to every entry.
 * Calls in flight: the per-frame view records and accumulator slots come from a ring in the context (4 096 frames) and stay a
 * call's own until its launch is over; a call that would reuse entries of an earlier call, on whatever stream, first waits on
 * the host for that call (batches of up to 2 048 frames never wait for the call just before them).  The first call with more
 * than 4 096 views, and every later call with more than any before, replaces the ring: the device is synchronised, so THAT
 * call is not asynchronous.
 * Cost of d_acc: every wave of a frame ends with five device-scope atomics into one of the frame's 8 slots.  Sized for small
 * frames (a 256 x 256 frame: 128 flushes per slot); a 4K frame has 16 200 per slot, which serialise on the slot's cache line
 * (about a millisecond per frame): pass d_acc = NULL there, or use the single-frame entries.
 * Not one of the render entries: it neither consumes nor fires rm_render_attach_diagnostics and leaves
 * rm_scene_set_time's value alone.  Asynchronous on `stream` like the other device entries; rm_last_kernel names the
 * frames_kernel<...> instantiation.  RM_E_INVALID for a null job, null views with n_views > 0, n_views < 0 or > 65535 (one
 * grid dimension) or a non-finite angle or time -- checked before anything else; RM_E_NO_DEVICE on a host-only context;
 * RM_E_NO_SCENE before any scene; n_views == 0 is RM_OK and launches nothing.
 * Deliberately NOT used here: the v2 wave loop, the run-time compiled scene kernels, the lean octree kernel (its node table
 * and the origin-relative boxes belong to ONE camera position) and striping.  Every scene is served by the ahead-of-time
 * one-ray-per-lane kernels, which give the same bytes; options tile_w and v1_block apply.  Many small frames suit this
 * entry; for 4K frames prefer single-frame calls in flight on several streams. */
RM_API int rm_render_frames_device(rm_ctx *ctx, const rm_job *job, int32_t shader, const rm_view *views, int32_t n_views,
                                   void *d_depth, void *d_normal, void *d_sdf, void *d_iters, void *d_rgba, void *d_acc,
                                   void *stream);

/* The views of a camera sweep, host-only, no ctx: views[0] = Camera.setAngles(pitch, yaw) (pitch clamped, camera.ts:58-62),
 * views[k] = that state after k calls of Camera.rotateCamera(d_pitch, d_yaw) (camera.ts:26-31) -- sequential binary64
 * additions (yaw_k = yaw_{k-1} + d_yaw, never k * d_yaw) with the pitch clamp at every step -- and time_k = time0 + k * d_time.
 * RM_E_INVALID for a non-finite argument, n < 0 or null views with n > 0. */
RM_API int rm_sweep_views(double pitch, double yaw, double d_pitch, double d_yaw, double time0, double d_time, int32_t n,
                          rm_view *views);

/* ---- two renders of a view: difference image and statistics --------------------------- */

/* The reference's README plans "more detailed diagnostic data including comparing different algorithms"; today its user compares
 * two marchers or acceleration structures by eye, switching between the two heatmap shaders.  This entry compares two G-buffer
 * sets of the same frames on the device -- two calls of rm_render_tile_device / rm_render_frames_device that differ in algorithm,
 * acceleration structure, overshoot or step size, a scene before and after an edit, or the host's own CPU result against this
 * library's -- and needs no scene. */
typedef enum rm_compare_map {
    RM_CMP_MAP_NONE = -1,   /* statistics only */
    RM_CMP_MAP_SDF = 0, RM_CMP_MAP_ITERS = 1, RM_CMP_MAP_DEPTH = 2, RM_CMP_MAP_NORMAL = 3, RM_CMP_MAP_SURFACE = 4
} rm_compare_map;

typedef struct rm_frame_set { const void *depth, *normal, *sdf, *iters; } rm_frame_set;   /* layouts of the header's top comment */

/* "Surface" is the G-buffer's own notion: raymarcher.ts:97-105 stores the normal bytes (128,128,128) exactly when the normal is
 * the zero vector -- on a miss (depth >= MAX_DIST, where getNormal is skipped) or where the gradient is zero.  The depth byte
 * cannot tell a hit from a miss: t in [9.5, 10) rounds to the same 10 a miss stores. */
typedef struct rm_compare_stats {        /* 128 bytes, one per frame, everything B against A */
    uint64_t pixels;
    uint64_t sum_sdf_a, sum_sdf_b, sum_iters_a, sum_iters_b;   /* stored u16 values, as main.ts:534-543 sums them */
    uint64_t sum_abs_depth;                                    /* sum |depthB - depthA| */
    uint64_t surface_a, surface_b;                             /* pixels whose normal bytes are not (128,128,128) */
    uint64_t surface_only_a, surface_only_b;
    uint64_t depth_differs, normal_differs, counters_differ;   /* counters: sdf or iters differ */
    uint64_t b_cheaper, a_cheaper;                             /* sdfB < sdfA, sdfA < sdfB */
    uint32_t max_abs_depth, max_abs_normal;                    /* normal: max over pixels and the three channels */
} rm_compare_stats;

/* n_frames frames of width x rows pixels, device pointers, ONE launch, asynchronous on `stream` like the other device entries.
 * Frame k occupies elements [k * W * rows, (k + 1) * W * rows) of every buffer (x3 normal, x4 rgba): the layout
 * rm_render_frames_device writes; n_frames = 1 is a single tile.  Each of the four pairs (depth, normal, sdf, iters) may be
 * absent -- NULL in a AND in b -- and every field derived from an absent pair is 0 (pixels is always W * rows).
 *   map, gain  the difference image, pure integer, alpha 255.  SDF, ITERS, DEPTH: d = B - A of that buffer, m = min(|d| * gain, 255):
 *              d > 0 (m, 0, 0), d < 0 (0, m, 0), d == 0 (0, 0, 0) -- red: B has or costs more (the reference's heatmaps are red and
 *              green too, and use 5).  NORMAL: m from the largest absolute channel difference, (m, m, 0).  SURFACE: on both sides
 *              (96, 96, 96), on neither (0, 0, 0), only B (255, 0, 0), only A (0, 255, 0); gain is not used.  gain is 1 .. 255.
 *   d_rgba     W * rows * n_frames * 4 bytes, written as whole pixels; NULL only with RM_CMP_MAP_NONE
 *   d_stats    NULL, or n_frames records (8-byte aligned), each written completely by the launch: neither d_rgba nor d_stats
 *              needs a pre-clear, there is no initialising launch.  Exact integers: the same record whatever the launch shape.
 * width == 0, rows == 0 or n_frames == 0 is RM_OK: every one of the n_frames records is all zero, no image byte is written.
 * RM_E_INVALID -- checked before anything else -- for a null a or b, a negative size, n_frames > 65535 (one grid dimension), a
 * pair given on one side only, a map outside the enum or whose pair is absent, and with a map other than NONE a gain outside
 * 1 .. 255 or a null d_rgba; also for an sdf / iters pointer that is not 2-byte or a d_stats that is not 8-byte aligned.
 * RM_E_NO_DEVICE on a host-only context; never RM_E_NO_SCENE.  Not a render entry: it neither consumes nor fires
 * rm_render_attach_diagnostics.  rm_last_kernel names the compare_kernel<map, stats> instantiation.
 * Calls in flight: a frame of more than one workgroup (above 4 096 pixels) combines per-workgroup partial records through a ring
 * in the context (4 096 records); a call owns its entries until its launch is over, on whatever stream it ran, and a call that
 * would reuse them waits on the host for it first -- the rule of rm_render_frames_device's ring.  No call needs more than half of it. */
RM_API int rm_compare_frames_device(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames,
                                    const rm_frame_set *a, const rm_frame_set *b,
                                    int32_t map, int32_t gain, void *d_rgba, void *d_stats, void *stream);
/* Same with host buffers (synchronous), staged through the context's scratch buffer. */
RM_API int rm_compare_frames(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames,
                             const rm_frame_set *a, const rm_frame_set *b,
                             int32_t map, int32_t gain, uint8_t *rgba, rm_compare_stats *stats);

/* ---- counter distributions per frame: histograms, percentiles, ranged heatmaps -------- */

/* The reference's two heatmap shaders colour by counter * 5 % 256 (IterationHeatmap.ts:24, SDFHeatmap.ts:24) and its README
 * warns that they "loop around": a pixel of 52 iterations looks like one of 1.  Its diagnostics are a sum, a maximum and a
 * minimum (main.ts:528-548), which the background pixels of a frame swamp.  These entries give, on the device and for a batch of
 * frames per launch, the histogram of each counter of each frame over all, the surface or the background pixels, two percentiles
 * derived from it, and a heatmap scaled to a range -- the arguments' or those two percentiles' -- that never wraps.  Neither
 * needs a scene. */
#define RM_HIST_BINS 256
typedef enum rm_hist_mask { RM_HIST_ALL = 0, RM_HIST_SURFACE = 1, RM_HIST_BACKGROUND = 2 } rm_hist_mask;

struct rm_counter_hist {              /* 1064 bytes; named by its tag only: rm_counter_hist is also the host entry below */
    uint64_t pixels;                  /* pixels the mask selects */
    uint64_t sum;                     /* of their stored u16 values */
    uint32_t min, max;                /* of their stored values; 0, 0 when pixels == 0 */
    uint32_t range_lo, range_hi;      /* the two requested percentiles, rule below */
    uint32_t shift, reserved;         /* the call's bin_shift; 0 */
    uint32_t bins[RM_HIST_BINS];
};
typedef struct rm_frame_hist { struct rm_counter_hist sdf, iters; } rm_frame_hist;   /* 2128 bytes, one per frame */

/* n_frames frames of width x rows pixels, device pointers, ONE launch, asynchronous on `stream`.  Frame k occupies elements
 * [k * W * rows, (k + 1) * W * rows) of every buffer (x3 normal): the layout rm_render_frames_device writes and
 * rm_compare_frames_device reads; n_frames = 1 is a single tile.
 *   mask         RM_HIST_ALL: every pixel; d_normal may be NULL and is not read.  RM_HIST_SURFACE / RM_HIST_BACKGROUND: the pixels
 *                whose normal bytes are not / are (128,128,128) -- "surface" as defined for rm_compare_stats; d_normal is needed.
 *   bin_shift    0 .. 8: bin(v) = min(v >> bin_shift, 255).  Shift 8 covers every u16 value exactly; with smaller shifts the last
 *                bin also holds everything above it.
 *   d_sdf, d_iters  either may be NULL, not both; the record of an absent counter is all zero except `shift`.
 *   lo_permille, hi_permille  0 <= lo <= hi <= 1000.  With M = pixels and a given p: r = floor(p * (M - 1) / 1000) in 64 bits, b_p
 *                the smallest b with bins[0] + .. + bins[b] > r.  range_lo = max(min, b_lo << shift); range_hi = max when
 *                b_hi == 255, else min(max, ((b_hi + 1) << shift) - 1).  M == 0: both 0.  range_lo <= range_hi always; with shift 0
 *                and values below 255 they are the exact nearest-rank percentiles; 0 and 1000 give min and max.
 *   d_hist       n_frames rm_frame_hist records (8-byte aligned), each written whole by the launch: no pre-clear, no
 *                initialising launch, no memset on the caller's side.  Exact integers: the same bytes whatever the launch shape.
 * width == 0, rows == 0 or n_frames == 0 is RM_OK: every one of the n_frames records is zero except `shift`.
 * RM_E_INVALID -- checked before anything else -- for a null d_hist or both counters null; a negative size, W * rows > UINT32_MAX
 * or n_frames > 65535 (one grid dimension); a mask outside the enum, or one other than ALL without d_normal; a shift or permille
 * out of range; a counter pointer that is not 2-byte or a d_hist that is not 8-byte aligned.  RM_E_NO_DEVICE on a host-only
 * context; never RM_E_NO_SCENE.  Not a render entry: it neither consumes nor fires rm_render_attach_diagnostics.  rm_last_kernel
 * names the hist_kernel<masked> instantiation.
 * Calls in flight: a frame of more than one workgroup (above 4 096 pixels) adds into a scratch entry of a ring in the context
 * (2 048 entries of 2 096 bytes, one per such frame; a call takes at most 1 024, half of it); a call owns its entries until its
 * launch is over, on whatever stream it ran, and only a call that would reuse the entries of a call still in flight waits on the
 * host for it first -- the rule of rm_compare_frames_device's ring.  Frames of one workgroup use no entry. */
RM_API int rm_counter_hist_device(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames,
                                  const void *d_sdf, const void *d_iters, const void *d_normal,
                                  int32_t mask, int32_t bin_shift, int32_t lo_permille, int32_t hi_permille,
                                  void *d_hist, void *stream);
/* Same with host buffers (synchronous), staged through the context's scratch buffer. */
RM_API int rm_counter_hist(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames,
                           const uint16_t *sdf, const uint16_t *iters, const uint8_t *normal,
                           int32_t mask, int32_t bin_shift, int32_t lo_permille, int32_t hi_permille,
                           rm_frame_hist *hist);

/* The heatmap of one counter scaled to a range, ONE launch for n_frames frames (layout as above, x4 rgba), asynchronous on
 * `stream`.  Per pixel value v: s = 0 if v <= lo, 255 if v >= hi, else (v - lo) * 255 / (hi - lo) by integer division; the colour
 * is R = min(2s, 255), G = min(512 - 2s, 255), B = 0, A = 255 -- the ramp of IterationHeatmap.ts:26-29 with s in place of
 * counter * 5 % 256, so lo = 0, hi = 51 reproduces the reference's heatmap wherever that one does not wrap.
 *   counter      0: d_counter holds sdfEval, 1: iters (decides which record of a frame gives the range)
 *   d_hist       NULL: every frame uses the arguments lo, hi (lo > hi is invalid).  Else n_frames rm_frame_hist records: frame k
 *                takes range_lo, range_hi of d_hist[k].sdf or .iters, read ON THE DEVICE -- the launch may follow
 *                rm_counter_hist_device on the same stream with no host synchronisation between them; lo and hi are ignored.
 *   d_rgba       W * rows * n_frames * 4 bytes, written as whole pixels; no pre-clear.  Without a pixel or a frame no byte is written.
 * RM_E_INVALID -- checked before anything else -- for a null d_rgba or d_counter, a counter other than 0 and 1, a negative size,
 * W * rows > UINT32_MAX, n_frames > 65535, lo > hi without d_hist, a d_counter that is not 2-byte or a d_hist that is not 8-byte
 * aligned.  RM_E_NO_DEVICE on a host-only context; never RM_E_NO_SCENE; not a render entry.  rm_last_kernel: shade_ranged_kernel.
 * Uses no ring: no call waits. */
RM_API int rm_shade_ranged_device(rm_ctx *ctx, int32_t counter, int32_t width, int32_t rows, int32_t n_frames,
                                  const void *d_counter, const void *d_hist, uint32_t lo, uint32_t hi,
                                  void *d_rgba, void *stream);
/* Same with host buffers (synchronous); hist is a host rm_frame_hist array or NULL. */
RM_API int rm_shade_ranged(rm_ctx *ctx, int32_t counter, int32_t width, int32_t rows, int32_t n_frames,
                           const uint16_t *values, const rm_frame_hist *hist, uint32_t lo, uint32_t hi,
                           uint8_t *rgba);

/* PhongModel.shade (phongModel.ts:33-72, as RM_SHADE_PHONG restates it) with the two terms of a light query, ONE launch for
 * n_frames frames (layout as rm_shade_ranged_device: frame k at element k * W * rows of every buffer, x3 normal, x4 rgba),
 * asynchronous on `stream`.  One line changes: I = min((0.1 + diff s + spec s) a, 1) with s = (double)lit[i] and
 * a = (double)ao[i], evaluated in that order, so s = a = 1 gives RM_SHADE_PHONG's bytes exactly.  Background pixels
 * (depth byte 255) keep PhongModel's (10, 10, 20, 255).  d_lit, d_ao: f32, what rm_ray_light writes for the frame's rays.
 * RM_E_INVALID -- checked before anything else -- for a null buffer, a negative size, W * rows > UINT32_MAX,
 * n_frames > 65535, a d_lit or d_ao that is not 4-byte aligned.  RM_E_NO_DEVICE on a host-only context; never
 * RM_E_NO_SCENE; not a render entry.  Without a pixel or a frame no byte is written.  rm_last_kernel: shade_lit_kernel.
 * Uses no ring: no call waits. */
RM_API int rm_shade_lit_device(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const void *d_depth,
                               const void *d_normal, const void *d_lit, const void *d_ao, void *d_rgba, void *stream);
/* Same with host buffers (synchronous). */
RM_API int rm_shade_lit(rm_ctx *ctx, int32_t width, int32_t rows, int32_t n_frames, const uint8_t *depth,
                        const uint8_t *normal, const float *lit, const float *ao, uint8_t *rgba);

/* The slice image of a field query, ONE launch, asynchronous on `stream`: n values -> n pixels.  d_values is f64[n] (dist)
 * for RM_FIELD_MAP_DISTANCE and u32[n] (count) for RM_FIELD_MAP_COUNT; d_rgba is 4n bytes, written as whole pixels with alpha
 * 255, no pre-clear.
 *   DISTANCE, per value d:  1. d is NaN: (255, 0, 255).  2. a = |d|; a < line: (255, 255, 255), the zero line.
 *     3. x = a / range; s = 255 if x >= 1, else (int)(x * 255.0), truncating; I = 96 + 159 * s / 255.
 *     4. y = a / band; q = (int)y if y < 2147483648.0, else 0; q odd: I = I * 3 / 4 -- every second iso-band is darker.
 *     5. the base colour is (60, 120, 230) if d < 0 (inside), else (230, 140, 50); -0.0 counts as outside.
 *     6. each channel is base * I / 255.  x and y are binary64 quotients; every other division is integer division.
 *   COUNT, per value v: s = 0 if v <= lo, 255 if v >= hi, else (v - lo) * 255 / (hi - lo) in 64 bits, and the ramp of
 *     rm_shade_ranged_device: R = min(2s, 255), G = min(512 - 2s, 255), B = 0.
 * RM_E_INVALID -- checked before anything else -- for a null argument, n < 0, a map outside the enum, reserved != 0, for
 * DISTANCE a non-finite or non-positive range or band or a non-finite or negative line, for COUNT lo > hi, a d_values that is
 * not 8-byte (DISTANCE) or 4-byte (COUNT) aligned.  RM_E_NO_DEVICE on a host-only context; never RM_E_NO_SCENE; n == 0 is
 * RM_OK.  Not a render entry; uses no ring: no call waits.  rm_last_kernel: shade_field_kernel. */
typedef enum rm_field_map { RM_FIELD_MAP_DISTANCE = 0, RM_FIELD_MAP_COUNT = 1 } rm_field_map;
typedef struct rm_field_shade {   /* 40 bytes */
    int32_t  map, reserved;       /* rm_field_map; 0 */
    double   range;               /* DISTANCE: |d| at which the intensity saturates; finite, > 0 */
    double   band;                /* DISTANCE: width of an iso-band; finite, > 0 */
    double   line;                /* DISTANCE: half-width of the white zero line; finite, >= 0 */
    uint32_t lo, hi;              /* COUNT: ramp range, lo <= hi */
} rm_field_shade;
RM_API int rm_shade_field_device(rm_ctx *ctx, const rm_field_shade *shade, int64_t n, const void *d_values, void *d_rgba,
                                 void *stream);
/* Same with host buffers (synchronous), staged through the context's scratch buffer. */
RM_API int rm_shade_field(rm_ctx *ctx, const rm_field_shade *shade, int64_t n, const void *values, uint8_t *rgba);

/* Multi-GPU sharding of one Job (replaces the contiguous ceil(H/N) split of main.ts:444-449
 * by a load-balanced one): the rows [y_start, y_end) are cut into stripes of `stripe_rows`
 * rows dealt round-robin over `n_parts`; this call renders, in ONE launch, the stripes of
 * `part`, packed in increasing y (rm_stripe_rows rows of `width` pixels).  Pixels are pure
 * functions of (x, y, W, H, camera, scene) (raymarcher.ts:72-76,83), so any row subset is exact. */
RM_API int rm_render_stripes_device(rm_ctx *ctx, const rm_job *job, int32_t shader, int32_t stripe_rows,
                                    int32_t n_parts, int32_t part, void *d_depth, void *d_normal,
                                    void *d_sdf, void *d_iters, void *d_rgba, void *stream);
/* number of rows part `part` owns (>= 0), or RM_E_INVALID */
RM_API int rm_stripe_rows(int32_t y_start, int32_t y_end, int32_t stripe_rows, int32_t n_parts, int32_t part);

/* Weighted deal of the stripes of `rows` rows over n_parts parts (replaces the equal ceil(H/N) shares of
 * main.ts:444-449 when the parts are NOT equally loaded: the root of the gather also reassembles the frame, so it
 * gets a smaller share).  owner[s] receives the part of stripe s (s < ceil(rows / stripe_rows) = the return value);
 * weights[p] > 0 are relative shares (NULL: equal).  Smooth weighted round-robin: every part's stripes stay spread
 * over the whole frame (load balance: the top and bottom of a frame are mostly root-box misses), and equal weights
 * give exactly the round-robin deal of rm_render_stripes_device.  Deterministic integer arithmetic: every rank
 * computes the same deal from the same weights.  Host-side, no ctx. */
RM_API int rm_deal_stripes(int32_t rows, int32_t stripe_rows, int32_t n_parts, const int32_t *weights, int32_t *owner);

/* One launch for an explicit list of stripes: stripe_ids[0 .. n_stripes) (strictly increasing, host memory, copied),
 * stripe k of the list being rows [y_start + id * stripe_rows, ...) of the Job, packed in list order.  Buffers must
 * hold the rows the list covers (the frame's last stripe may be partial). */
RM_API int rm_render_stripe_list_device(rm_ctx *ctx, const rm_job *job, int32_t shader, int32_t stripe_rows,
                                        const int32_t *stripe_ids, int32_t n_stripes, void *d_depth, void *d_normal,
                                        void *d_sdf, void *d_iters, void *d_rgba, void *stream);

/* Rank 0's fan-in (replaces `buffer.set(tile, yStart * width)` per worker result, main.ts:461-468, and the combined
 * diagnostics of main.ts:528-548) as ONE kernel: d_gathered holds `world` per-rank packed buffers rank_stride bytes
 * apart (what a gather delivers); the section at section_offset of each holds that rank's stripes, packed in
 * increasing y, rows of row_bytes = width * bytes-per-pixel.  owner[s] (host, n_stripes = ceil(height / stripe_rows)
 * entries, as rm_deal_stripes returns them) names the rank of frame stripe s.  Writes the row-major frame to d_frame.
 * acc_offset >= 0: each rank's 32-byte partial diagnostics accumulator (rm_reduce_counters_enqueue layout) sits at
 * that offset of its packed buffer; their combination is written to d_acc (acc_offset < 0 or d_acc NULL: skipped). */
RM_API int rm_assemble_frame_device(rm_ctx *ctx, const void *d_gathered, int64_t rank_stride, int64_t section_offset,
                                    int32_t row_bytes, int32_t height, int32_t stripe_rows, const int32_t *owner,
                                    int32_t n_stripes, int32_t world, void *d_frame, int64_t acc_offset, void *d_acc,
                                    void *stream);

/* Replaces ShadingModel.shade(shaded, depth, normal, sdfEval, iters, width, height)
 * (shadingModel.ts:8-17 and the four models), host buffers. */
RM_API int rm_shade(rm_ctx *ctx, int32_t shader, int32_t width, int32_t height,
                    const uint8_t *depth, const uint8_t *normal, const uint16_t *sdf,
                    const uint16_t *iters, uint8_t *rgba);
RM_API int rm_shade_device(rm_ctx *ctx, int32_t shader, int32_t width, int32_t height,
                           const void *d_depth, const void *d_normal, const void *d_sdf,
                           const void *d_iters, void *d_rgba, void *stream);

/* Replaces the diagnostics pass of main.ts:528-548. */
RM_API int rm_reduce_counters(rm_ctx *ctx, const uint16_t *sdf, const uint16_t *iters, int64_t n,
                              rm_diagnostics *out);
/* device buffers; result written to host `out` after a stream sync */
RM_API int rm_reduce_counters_device(rm_ctx *ctx, const void *d_sdf, const void *d_iters, int64_t n,
                                     rm_diagnostics *out, void *stream);

/* Asynchronous form for a frame loop: enqueues init + reduction on `stream` and leaves the
 * result in device memory `d_acc` (32 bytes: u64 total_sdf, u64 total_iters, u32 max_sdf,
 * u32 min_sdf, u64 pad); no host synchronisation. */
RM_API int rm_reduce_counters_enqueue(rm_ctx *ctx, const void *d_sdf, const void *d_iters, int64_t n,
                                      void *d_acc, void *stream);

/* The same diagnostics WITHOUT a second pass over the counters: the next render call on this context
 * (rm_render_tile_device, rm_render_stripes_device or rm_render_stripe_list_device) also leaves, in device memory
 * `d_acc` (32 bytes, 8-byte aligned, the layout of rm_reduce_counters_enqueue), the sum / max / min of the sdfEval
 * values and the sum of the iteration values of exactly the pixels it renders -- as stored, Uint16Array wrap included
 * (raymarcher.ts:79-80,119; main.ts:534-543).  The render kernel accumulates them from the registers it stores the
 * counters from and its last wave writes the result: no initialisation of d_acc, no further launch, and the counter
 * buffers themselves may be NULL.  A call that renders no pixel writes the neutral elements (sums 0, max 0, min
 * UINT32_MAX).  One-shot: consumed by the next render call whether it succeeds or not; d_acc = NULL cancels. */
RM_API int rm_render_attach_diagnostics(rm_ctx *ctx, void *d_acc);

/* ---- tile partition (main.ts:444-450) ------------------------------------------- */

/* rows of worker i of n: [min(i*r, H), min((i+1)*r, H)) with r = ceil(H / n) */
RM_API int rm_partition_rows(int32_t height, int32_t n_workers, int32_t i, int32_t *y_start,
                             int32_t *y_end);

/* ---- device numerics self-test (parity aid, not part of the reference surface) ---- */

/* V8 Math.hypot of n float triples evaluated by the device code path used in Sphere.sdf */
RM_API int rm_selftest_hypot(rm_ctx *ctx, const float *xyz, int64_t n, double *out);

/* JS Math.* as the device computes them (csrc/rm_jsmath.h, fdlibm restated like V8's ieee754.cc):
 * fn 0 sin, 1 cos, 2 atan2(a, b), 3 asin, 4 log, 5 pow(a, b), 6 round, 7 atan; b may be NULL. */
RM_API int rm_selftest_jsmath(rm_ctx *ctx, int32_t fn, const double *a, const double *b, int64_t n, double *out);

/* V8 Math.hypot of n binary64 triples (xyz f64[3n]) as the scene builders evaluate it for BoundingBox.distanceTo
 * (boundingBox.ts:46): on_device 0 = the host builder's own function (works on a host-only context), 1 = the device
 * builder's (csrc/rm_scene_build.hip, hypot3_f64).  The two agree bit for bit. */
RM_API int rm_selftest_hypot64(rm_ctx *ctx, const double *xyz, int64_t n, int32_t on_device, double *out);

/* Device check of the shared-reciprocal division used by the v2 kernel's sphere SDF: evaluates
 * Math.hypot with the compiler's IEEE divisions and with the shared reciprocal on n generated
 * binary32 triples (zeros, denormals, equal magnitudes included) and counts bitwise mismatches. */
RM_API int rm_selftest_fastdiv(rm_ctx *ctx, uint64_t seed, int64_t n, uint64_t *mismatches);

/* Device self-test of the range-restricted division of ray set-up (rm_device.h div_in_range) against the compiler's IEEE
 * division, EXHAUSTIVE over its domain: mode 0 = 1.0 / d for every finite non-zero binary32 d; mode 1 = x / W for all
 * integers 0 <= x < 65536, 1 <= W < 65536.  Counts bitwise mismatches (2^32 cases per mode, about a second). */
RM_API int rm_selftest_recip(rm_ctx *ctx, int mode, uint64_t *mismatches);

/* Diagnostic builds only (make EXTRA=-DRM_STAMPS): reads and clears eight per-section cycle
 * accumulators of the v2 wave loop (all zero in the product build). */
RM_API int rm_debug_read_stamps(rm_ctx *ctx, uint64_t *out8);

/* Run-time specialisation of expression forests (option `specialise`, default 1).  The reference evaluates an operator tree
 * by virtual dispatch (src/util/primitives/primitive.ts:33-39 and the overrides in src/util/primitive_operations/ *.ts); here the
 * active scene's trees are emitted as straight-line HIP and compiled for gfx950 with hiprtc into the one-ray-per-lane kernels,
 * once per (acceleration structure, marcher family) the scene is rendered with, at the first such render (1.5 - 3 s,
 * synchronous); loaded kernels are cached for the life of the process (up to 256, keyed by the generated source), so a scene
 * that comes back -- a preset menu -- does not compile again.  Without libhiprtc.so, for forests above 32 objects / 512 instructions, or with `specialise` = 0 the device
 * interpreter serves the scene (same results: both call the same formula functions in the same order).
 *   rm_rtc_source         the generated source of the active scene (NUL-terminated, truncated to cap; *needed = full size)
 *   rm_rtc_compile_check  compiles it for (accel, other != 0: the marchers other than the sphere tracer) without loading the
 *                         result -- works on a host-only context; log receives the compiler's resource-usage remarks.
 *                         A kernel that spills a VGPR (in rm_rtc_render or rm_rtc_distance) is never loaded: a render would
 *                         record the compile as failed and launch the interpreter kernel.  This call applies the same rule:
 *                         it returns RM_E_UNSUPPORTED and the log starts with "refused: <function> spills N VGPRs" (the
 *                         compiler's remarks follow); RM_E_INVALID is a compile error
 *   rm_rtc_status         kernels compiled / failed for the active scene and the log of the compile behind the most recent kernel
 *                         lookup -- also when the kernel or the refusal came from the process-wide cache (or why hiprtc is absent) */
RM_API int rm_rtc_source(rm_ctx *ctx, char *out, int64_t cap, int64_t *needed);
RM_API int rm_rtc_compile_check(rm_ctx *ctx, int32_t accel, int32_t other, char *log, int64_t cap, double *seconds);
RM_API int rm_rtc_status(rm_ctx *ctx, int32_t *compiled, int32_t *failed, char *log, int64_t cap);

/* Diagnostic builds only (make EXTRA=-DRM_COUNTS): reads and clears the execution counts of sixteen events of the
 * v2 wave loop (scripts/counts.py) or of the v1 octree kernels (scripts/counts_v1.py) -- out32[i] wave-level executions, out32[i + 16] lanes active in them (all zero in the product build). */
RM_API int rm_debug_read_counts(rm_ctx *ctx, uint64_t *out32);
/* The item durations (units of 2.56 us, one byte per work item: 64 queues x 4096 slots) the last v2 launch recorded for the
 * longest-first order of the next one (option lpt); scripts/lpt_costs.py. */
RM_API int rm_debug_read_lpt_costs(rm_ctx *ctx, uint8_t *out, int64_t n);
/* One table of the active scene, for tests of the scene builders: `name` is a scene array as csrc/rm_api.cpp lists them
 * (RM_SCENE_ARRAYS: spheres, radii, bvh, bvh_prims, oct, oct_prims, pq_cells, pq_list, nn_cells, nn_list, prims, prog,
 * obj_ranges, oct_recs, oct_lut, oct_sub_hdr, oct_sub_list, slot_object, ext_cells, ext_list, step_tab).  *bytes always receives the
 * array's size; the bytes are copied to `out` only if cap holds them.  from_device != 0: the device copy, read after a device
 * synchronise (RM_E_NO_DEVICE on a host-only context); 0: the host builder's copy.  RM_E_INVALID for an unknown name,
 * RM_E_NO_SCENE before any scene. */
RM_API int rm_debug_scene_table(rm_ctx *ctx, const char *name, int32_t from_device, void *out, int64_t cap, int64_t *bytes);
/* Option min_fill (below), for tests and evidence.  rm_debug_launch_fill: *effective = the workgroups per CU a v2 launch
 * brings when blocks_per_cu is `asked` (1..8), with the context's min_fill and queue count; works on a host-only context.
 * rm_debug_last_launch: the last launch of the v2 wave loop -- out[0] workgroups, out[1] threads per workgroup, out[2]
 * dynamic LDS bytes (zeros before the first such launch) -- and out[3] the context's CU count. */
RM_API int rm_debug_launch_fill(rm_ctx *ctx, int32_t asked, int32_t *effective);
RM_API int rm_debug_last_launch(rm_ctx *ctx, uint32_t out[4]);
/* Option overlap_fill (below), for tests and evidence: the counterpart of rm_debug_launch_fill with both stages --
 * *effective = the workgroups per CU a v2 launch brings for a frame of `items` work items when blocks_per_cu is `asked`
 * (1..8); works on a host-only context (256 CUs). */
RM_API int rm_debug_overlap_fill(rm_ctx *ctx, int32_t asked, int64_t items, int32_t *effective);
/* Option step_box (below), for tests and evidence; works on a host-only context except for out[0].  out[0]: whether the last
 * launch of the v2 wave loop tested its in-round march steps against the scene's step-box table (0 before the first such
 * launch); out[1]: whether a launch of the active scene would, with the options as they stand -- the launcher's own decision;
 * out[2]: why not (0: it would; 1: the options step_box, multi_step or kernel, or the kind of scene; 2: the scene has no table --
 * more than 62 distinct thresholds on an axis, or a face coordinate that is non-zero and below 1e-30 in magnitude; 3: the table
 * would cost LDS that the launch keeps for the scene, the origin-relative boxes or a workgroup per CU); out[3]: the hit-list
 * capacity that launch gets, out[4]: what it would get with step_box 0; out[5]: the table's size in bytes (0: none). */
RM_API int rm_debug_step_box(rm_ctx *ctx, int32_t out[6]);
/* Option cell_tab (below), for tests and evidence; works on a host-only context except for out[0].  out[0]: whether the last
 * launch of the v2 wave loop read its candidate spheres from the scene's cell table (scene table "cell_tab"; 0 before the first
 * such launch); out[1]: whether a launch of the active scene would, with the options as they stand; out[2]: why not (0: it
 * would; 1: the options cell_tab, step_box, multi_step or kernel, the kind of scene, or a launch that does not take the
 * step-box table; 2: the scene has no table -- no step-box table, more than 4 096 threshold cells, a cell with more than 255
 * spheres, a primitive that is not a sphere; 3: the table would cost the launch a workgroup per CU, entries of its hit lists or
 * its staging); out[3]: the hit-list capacity that launch gets, out[4]: what it would get with cell_tab 0; out[5]: the table's
 * size in bytes (0: none); out[6]: the workgroups of that launch a CU holds; out[7], out[8]: the bytes of scene tables the
 * launch stages in LDS, and would with cell_tab 0; out[9..11]: the table's cells, records and distinct leaf sets. */
RM_API int rm_debug_cell_tab(rm_ctx *ctx, int32_t out[12]);
/* Option runner_up (below), for tests and evidence; works on a host-only context except for out[0].  out[0]: whether the last
 * launch of the v2 wave loop bounded the runner-up sphere of an in-round march step by its own distance (0 before the first such
 * launch); out[1]: whether a launch of the active scene would, with the options as they stand; out[2]: why not (0: it would;
 * 1: option runner_up is 0; 2: the launch does not take the cell table -- rm_debug_cell_tab says why; 3: the scene's spheres do
 * not share one radius, or option uniform is 0); out[3]: 0. */
RM_API int rm_debug_runner_up(rm_ctx *ctx, int32_t out[4]);
/* The key update of the one-radius scan, the text the wave loop runs, over a caller's n keys (a squared distance's bit pattern,
 * the sphere id in its low byte); needs no context and no device.  out3: the three smallest keys in order, equal keys counted as
 * often as they came, 0xFFFFFFFF where there are fewer; *lb3: the lower bound the third key gives the spheres behind the
 * runner-up for radius rf, +infinity exactly when fewer than three keys came; *lb3_carried: that bound as the in-round march steps
 * read it, cut to the upper half of a word on its way (never above *lb3, at least 0.97 of a positive one).  keys may be null when
 * n is 0. */
RM_API int rm_debug_scan_keys(const uint32_t *keys, int64_t n, float rf, uint32_t out3[3], float *lb3, float *lb3_carried);
/* Option exact (below), for tests and evidence; works on a host-only context.  What the next exact query of the active scene
 * walks -- out[0]: 0 every object, 1 the scene's BVH, 2 an exact tree of its own -- and that tree's nodes (out[1]), leaves
 * (out[2]) and depth (out[3]); zeros in mode 0.  It builds the exact tree if it is due (and, with a device, copies it up),
 * whatever the option says.  RM_E_NO_SCENE without a scene. */
RM_API int rm_debug_exact_tree(rm_ctx *ctx, int32_t out[4]);
/* Option rect_cull (below), for tests and evidence; both work on a host-only context (except for out[0]).  rot9 / origin3: a
 * camera as rm_camera_from_angles gives it; width x height: the full frame.
 * rm_debug_rect_cull -- out[0]: whether the last launch of the v2 wave loop culled its batches' leaves by screen rectangles (0
 * before the first such launch); out[1]: whether a launch of the active scene with this camera and frame would; out[2]: why not
 * (0: it would; 1: the options rect_cull, cull or kernel, or the kind of scene; 2: more leaves than out[4]; 3: the columns of
 * rot9 are not orthonormal within 1e-6, the camera is not finite, or a side of the frame exceeds 65 536 pixels); out[3]: the
 * leaves in the cull's table; out[4]: the most a launch keeps rectangles for.
 * rm_debug_leaf_rects -- the table the workgroups of such a launch fill, from the same text, on the host: per leaf the
 * inclusive pixel bounds x_lo, x_hi, y_lo, y_hi (four uint16; whole frame 0, 65535, 0, 65535; no pixel 65535, 0, 65535, 0) of
 * every pixel whose ray can hit the leaf's box, and in nodes[] the leaf's index in the scene's BVH table.  *n: the leaves, of
 * which the first `cap` are written; 0 when the launch would take the plane cull.  rects and nodes may be null. */
RM_API int rm_debug_rect_cull(rm_ctx *ctx, const float *rot9, const float *origin3, int32_t width, int32_t height, int32_t out[5]);
RM_API int rm_debug_leaf_rects(rm_ctx *ctx, const float *rot9, const float *origin3, int32_t width, int32_t height,
                               uint16_t *rects, int32_t *nodes, int64_t cap, int64_t *n);
/* Diagnostic builds only (make EXTRA=-DRM_STAMPS): start and end time (100 MHz ticks) of the first 8192 waves of the last
 * v2 launch -- out[w] start of the wave loop, out[8192 + w] end, out[16384 + w] kernel entry, 0 where no wave ran
 * (scripts/tail_hist.py). */
RM_API int rm_debug_read_wave_times(rm_ctx *ctx, uint64_t *out24576);
/* Diagnostic builds only (EXTRA="-DRM_STAMPS -DRM_STAMPS_LOG"): low 32 bits of the 100 MHz clock at the start of the first 96
 * batches of the first 2048 waves of the last v2 launches, out[wave * 96 + k]; 0 = no such batch (scripts/batch_timeline.py). */
RM_API int rm_debug_read_batch_log(rm_ctx *ctx, uint32_t *out196608);

/* Kernel-variant knobs for measurement; unknown keys or values are RM_E_INVALID.  They NEVER change results
 * (tests/test_gpu_parity.py renders every combination and compares the bytes).
 *   kernel 0 auto | 1 one ray per lane (v1) | 2 uniform wave loop (v2)      tile_w 8|16|32|64 pixels per wave row
 *   filter 0|1 conservative binary32 bound before exact evaluations         coop 0|1 wave-cooperative all-primitive loop
 *   nodes_in_lds 0|1 scene tables staged in LDS (v2)                        list_cap 1..64 hit-leaf list entries per ray (v2)
 *   grid 0|1 leaf grid for BVH.getPrimitivesAt (v2)                         nn 0|1|2 nearest-candidate grid off|on|auto
 *   ext 0|1       BVH (v2): all-primitive evaluations outside the root box scan the exterior candidate grid's cell list (default 1)
 *   device_build 0|1  rm_scene_edit_spheres: the pair loops of the scene build on the device (default 1; 0: the host builder
 *                 for everything -- the A/B baseline; same tables either way; never read by the upload entries)
 *   recs, lut, sub 0|1 octree: leaf-ordered records, findNode cell table, sub-cell candidate lists
 *   blocks_per_cu 1..8, refill 1..64, hw_xcd 0|1, item_px 64|128|256       persistent-kernel scheduling (v2)
 *   static 0..95 percent of every tile queue assigned to the waves without atomics (v2; for overlapping frames)
 *   uniform 0|1   scenes whose spheres share one radius: rank leaf candidates by squared centre distance (v2, default 1)
 *   rel 0|1       BVH node boxes relative to the frame's ray origin, as doubles in LDS, when they fit (v2, default 1)
 *   cull 0|1      whole 64-pixel batches find their hit BVH leaves by a bundle-frustum cull (v2, <= 256 leaves, default 1)
 *   rect_cull 0|1 v2, with cull: a batch's candidate leaves come from comparing its pixel rectangle with a table of leaf screen
 *                 rectangles that every workgroup of the launch works out once for the launch's camera, and a batch without a
 *                 candidate sets up no ray (default 1; 0, more than 256 leaves (no bundle cull at all), or a camera whose axes are not orthonormal: four
 *                 bundle planes per batch and leaf; same bytes either way; rm_debug_rect_cull)
 *   lds_kb 0|16..64  LDS budget per workgroup the v2 launcher trims the per-ray hit lists to (0, default: as many workgroups per CU
 *                 as the kernel's registers allow -- six, 26 880 bytes each --, then five, then four; 32: five; 40: four)
 *   n0_batch 1..64 BVH (v2): getNormal is deferred until no lane of the wave needs a march distance, then evaluated for all waiting
 *                 rays in one round, the three offset samples taken from the sphere that gave d0 where provably the minimum;
 *                 lanes waiting that trigger that round early (64: never early; default 64)
 *   lpt 0|1       v2: hand out a launch's work items longest-first using the item durations the previous launch recorded (any
 *                 order gives the same bytes; default 1: a frame alone 1.07 against 1.14 ms; bench.py turns it off with frames in flight)
 *   multi_step 0|1  v2 BVH: a lane takes further march steps inside a round while the leaf set and the winning sphere provably
 *                 stay the same (default 1; same bytes either way)
 *   step_box 0|1  v2 BVH, those steps: the leaf set at the new point is known to be the round's when the point lies in the same
 *                 cell of the per-axis thresholds of the leaf boxes (lo, and the next binary32 above hi) as the round's point:
 *                 six compares against a bracket found once per run, instead of the cell's leaf list per step (default 1; 0, a
 *                 scene without the table, or a launch whose LDS has no room for it: the exact test; same bytes either way)
 *   cell_tab 0|1  v2 BVH, with step_box: a point's candidate spheres, their number and the box of those steps come from a table
 *                 over the cells of those thresholds (sphere scenes of at most 4 096 cells), found with one look-up per round,
 *                 instead of from box tests against the leaf grid's lists; the launch then stages the table in the leaf
 *                 grid's place (default 1; 0, a scene without the table, or a launch it does not fit: as before; same bytes
 *                 either way; rm_debug_cell_tab)
 *   runner_up 0|1 v2 BVH, those steps, in a launch that took the cell table of a scene whose spheres share one radius: a step
 *                 that the bound of all other candidates (the runner-up's bound at the round's point less the distance
 *                 travelled) does not admit is admitted when the runner-up sphere's own distance at the new point, and the
 *                 third-nearest candidate's bound less the distance travelled, both exceed the winner's exact distance; fewer
 *                 runs end, fewer rounds begin (default 1; 0, or any other launch: the one bound; same bytes either way;
 *                 rm_debug_runner_up)
 *   lds_fill 0|1  v2: pad the LDS request so that exactly blocks_per_cu workgroups fit a CU (default 0; measurement knob)
 *   min_fill 0|1  v2: a persistent launch brings max(blocks_per_cu, ceil(6 / Q)) workgroups per CU, Q = GPU_MAX_HW_QUEUES as
 *                 rm_create found it (unset or not a positive integer: 4, HIP's default; never set by the library).  Launches
 *                 on streams that share a hardware queue run one after the other, so no launch overlaps with more than Q - 1
 *                 others and a CU holds six of the wave loop's workgroups: fewer per launch leave wave slots empty whatever the
 *                 caller keeps in flight.  Q >= 6: as asked.  Q = 4: at least 2.  blocks_per_cu reads back as set and lds_fill
 *                 keeps going by it (default 1; 0 = exactly blocks_per_cu, for sweeps; same bytes either way)
 *   overlap_fill 0|1  v2, above that floor, Q < 6: streams are not dealt evenly over the hardware queues, so for part of every
 *                 burst fewer than Q launches run (Q = 4, twelve streams: 1.74 on average for 53 % of the busy time).  A launch
 *                 brings min(6, ceil(6 / (0.436 Q))) workgroups per CU -- Q = 4: 4 -- when each of its waves still gets 3 of
 *                 the frame's work items; smaller frames keep the floor (default 1; 0 = the floor alone; same bytes either way)
 *   item_wide 0|1 v2: the 64-pixel batches of a work item side by side (item = tile_w * item_px / 64 pixels wide) instead of one
 *                 above the other (default 0: measured no gain in write traffic, 2 % slower with frames in flight)
 *   specialise 0|1|2  small scenes: 1 (default) = the scene compiled into the kernel at run time (rm_rtc_* above), waiting for the
 *                 compile at the first render; 2 = the same without waiting -- a background thread compiles, the ahead-of-time
 *                 kernels render meanwhile (same bytes), the scene's own kernel takes over when it is ready; 0 = the
 *                 ahead-of-time kernels only (the device interpreter of csrc/rm_program.h for operator trees)
 *   specialise_v2_after 0..  the v2 wave loop: after this many launches with the same CONFIGURATION (frame size, shader, option
 *                 switches, the scene's counts and grids, tile geometry, LDS layout -- csrc/rm_v2_fields.h; not the camera, not
 *                 the rows of a launch) the kernel is compiled with that configuration's parameters as literals (~2 s; waiting
 *                 for it or not as `specialise` says) and used from then on: C3 at 4K 1 190 -> 1 310 frames/s.  Default 3;
 *                 0: never.  rm_last_kernel marks such launches "[launch constants compiled in]"
 *   rtc_spheres 0..33  sphere lists of fewer spheres than this (default 16) and primitive lists of up to 32 primitives are compiled
 *                 too, one single-leaf object per primitive, when their BVH has at most eight leaves (emitted as code: no node
 *                 walks in memory); they then run in the one-ray-per-lane kernel instead of the v2 wave loop
 *   prune 0|1     specialised kernels: smooth unions / subtractions over spheres, boxes and tori skip operands whose binary32
 *                 interval proves they cannot matter (exact: csrc/rm_rtc.cpp; default 1; read when a scene is built)
 *   v1_lists 0|1  v1 BVH kernels: per-ray hit-leaf lists (as v2) instead of one tree walk per interval advance (default 1)
 *   v1_block 64|128|256  v1 kernels: threads per workgroup (default 64: one wave, so wave slots refill one by one); without an
 *                 explicit tile_w the v1 kernels use 8 x 8-pixel wave tiles
 *   oct_lean 0|1  octree + sphere scene + sphere tracer: the lean kernel render_kernel_oct (march and getNormal as phases of one
 *                 loop, eight waves per SIMD, node boxes relative to the camera position from a per-camera table) instead of
 *                 render_kernel<1, false, 0> (default 1; needs recs, lut and filter on)
 * The two options that are NOT measurement knobs but part of the numeric contract:
 *   exact 0|1     the point, field, tile and mesh queries answer from the exact field instead of Scene.getDistance (default 0;
 *                 "the exact field" below has the rule; every other entry ignores it)
 *   length 0|1   gl-matrix vec3.length / vec3.distance (sphere.ts:12-14, box.ts:26,33, mandelbulb.ts:46, smoothUnion.ts:45):
 *                 0 = Math.hypot(x, y, z) (gl-matrix 3.0 - 3.4.3, default), 1 = Math.sqrt(x*x + y*y + z*z) (the form a later
 *                 3.4.x release may use).  Results differ by <= 1 ulp(f64) per distance; the active scene is
 *                 rebuilt (bounding radii of boxes and smooth unions use it too).
 *                 NOTE: the reference pins gl-matrix 3.4.4 (package.json:25), whose source is not available offline, while the
 *                 DEFAULT follows the formula of 3.0 - 3.4.3.  Nothing in the reference tree decides between the two (no
 *                 fixture, no test): parity is unpinned on this point.  Goldens, the cross-check shim and the benchmark exist
 *                 for both modes (tests/golden/, bench.py --opt length=1), so the default is a one-line change
 *                 (rm_api.cpp: opt_length) once the pinned version's formula is known.
 *
 * The exact field (option `exact` = 1).  Scene.getDistance is the marchers' bound: an empty octree leaf answers a constant, a
 * point inside some BVH leaf box is measured against those leaves only (an over-estimate, by any amount).  With exact = 1 the
 * distance function D(x) in the rules of the entries below is replaced by
 *     E(x) = min(10, min over ALL objects of Primitive.sdf(x))   at the query's time,
 * which is what rm_scene_distance returns, bit for bit, from a context that holds the same scene uploaded with acceleration
 * None, the same `length` option and the same time -- whatever acceleration the active scene has.  Everything else in each
 * rule is unchanged.
 *   rm_scene_points, rm_scene_points_device   D becomes E everywhere: the loop, the gradient G, dist and the object.  The
 *                 object's candidates are all objects: the lowest index with sdf == E under IEEE ==, the lowest NaN candidate
 *                 when E is NaN, -1 without a match.
 *   rm_scene_field, rm_scene_field_device     dist and dist32 come from E.
 *   rm_scene_tiles_device                     the tiles hold E, so rm_scene_mesh_sparse meshes E.
 *   rm_scene_mesh                             samples E (it goes through the field launch).
 * rm_scene_blocks_device uses the exact field with or without the option.  rm_scene_distance, rm_debug_wave_distance, every
 * render entry, rm_ray_march / _pick / _light / _walk and rm_shade_* ignore the option: they restate the reference's marchers,
 * which are defined on the bounded field.  With exact = 0 no entry changes a byte or a kernel name; with exact = 1
 * rm_last_kernel names point_kernel<EXACT, GEN>, field_kernel<EXACT, GEN> or tiles_kernel<EXACT, GEN> (the device symbols
 * are point_exact_kernel<GEN>, field_exact_kernel<GEN> and tiles_exact_kernel<GEN> for sphere and primitive records;
 * expression programs, which evaluate every object, run the acceleration-None instantiation <0, GEN> under that name).
 * How E is found depends on the scene (rm_debug_exact_tree reports it) and never changes its value.  Sphere and
 * primitive-record scenes under a BVH walk the scene's BVH with the pruning of the sparse mesher's coarse pass (skip a subtree
 * iff db * (1 - 2^-20) - 2^-20 > best: strict, so no pruned object ties the minimum) and one more condition, db > 0: inside a
 * box an sdf may be negative, as deep as the object is large, so a box that contains the point is never skipped -- a point
 * inside two overlapping spheres finds the deeper one.  (The coarse pass walks by the inequality alone, as it is written there.)  Octree and None scenes of such records
 * walk an EXACT TREE of their own, built by the BVH's rule over the same padded object boxes, on the host, at the first exact
 * query (or rm_debug_exact_tree) after the scene was made, and copied to the device once -- that one call is synchronous, also
 * for the _device entries -- and dropped by every change of the scene (an upload, a preset switch, rm_scene_edit_spheres, the
 * rebuild `length` triggers).  Pruning needs Primitive.sdf >= the distance to the object's padded box, which holds when the
 * sdf is a true world-space distance: every other scene -- expression forests, a primitive with a transform that is not rigid,
 * a negative radius or extent, an empty scene, a tree that would need a leaf of more than 255 objects -- evaluates every object.
 * Exact tiles cull the tree once per tile into a candidate list (csrc/rm_kernels.hip, tiles_kernel); the values are E bit for bit.
 *   count (points and field) is the number of Primitive.sdf evaluations the lane actually made: deterministic for a scene, a
 *                 point and the options, equal between the host and the _device entries, at most (objects) x (evaluations of
 *                 E), and exactly that product where every object is evaluated.  Its value under a tree is otherwise not part
 *                 of the contract. */
RM_API int rm_set_option(rm_ctx *ctx, const char *key, int64_t value);
RM_API int rm_get_option(const rm_ctx *ctx, const char *key, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* RM_RAYMARCH_H */
