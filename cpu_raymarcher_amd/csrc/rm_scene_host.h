// rm_scene_host.h -- host-side scene construction for the MI355X render path: sphere
// presets, camera matrices, BVH / Octree build and flattening into the device layout of
// rm_types.h.  Runs once per scene change (the reference rebuilds per tile per frame,
// raymarchWorker.ts:37-38).  Pure C++, no HIP.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "rm_types.h"

namespace rmh {

constexpr int kPresetCount = 19;  // sceneManager.ts:102-357
constexpr int kStepBoxCap = 62;   // distinct thresholds per axis a step-box table holds (with the two sentinels: 64 words)
// look-up bins per axis over the root extent, one byte each.  32, not more: the Dense Sphere Grid's table is then 240 bytes,
// and the 288 bytes its launch has left below the six-workgroups-per-CU budget hold it without a shorter hit list (13 entries);
// its thresholds are 0.15 apart at least, a bin is 0.089 wide, so a bin still holds one threshold at most
constexpr int kStepBoxBins = 32;
// threshold cells a cell table (build_cell_tab) may have: two bytes each, and the table must fit the LDS that the point-query
// grid frees in a launch that takes it (from that budget, not from a measurement)
constexpr int kCellTabCells = 4096;
// false (a measurement build, EXTRA=-DRM_CELL_TAB_SINGLE): every cell's box is the cell itself -- the arm that separates the
// table's two gains, the look-up in place of the box tests and the merged boxes
#ifdef RM_CELL_TAB_SINGLE
constexpr bool kCellTabMerge = false;
#else
constexpr bool kCellTabMerge = true;
#endif

// one primitive as the ABI hands it over (include/rm_raymarch.h: rm_prim)
struct PrimDesc {
    int type = 0;        // 0 sphere, 1 box, 2 torus
    float m[16];         // world -> local, gl-matrix layout
    double params[3];    // sphere: r; box: halfSize; torus: major, minor
};

// one node of an SDF expression forest as the ABI hands it over (include/rm_raymarch.h: rm_node).
// Operands must precede the node that uses them (a, b < own index).
struct NodeDesc {
    int type = 0;        // 0 sphere, 1 box, 2 torus, 3 mandelbulb, 10 round, 11 smooth union, 12 smooth subtraction,
                         // 13 twist, 14 repetition, 15 animated translate
    int a = -1, b = -1;  // operand node indices
    float m[16];         // leaves: world -> local.  Operators derive theirs (wrappers: the operand's; unions: identity)
    double params[6];    // see RmInstr::p
};

// The expression tree behind an object's instruction stream (HostScene::prog), for the run-time specialiser (rm_rtc.h):
// pre / main index the instructions of the node (-1: none -- an operator whose identity transform lets its operands read its
// own point has no PRE half; Twist / Repetition / AnimatedTranslate have no POST half), a / b the operand nodes.
struct ProgTreeNode {
    int pre = -1, main = -1, a = -1, b = -1;
};

struct HostScene {
    int accel = 0;
    int preset = 0;
    bool general = false;         // RmPrim records instead of RmSphere
    bool program = false;         // expression programs (RmInstr) instead of either
    int prog_slots = 1, prog_vals = 1;  // what the deepest program needs (device LDS sizing)
    std::vector<RmInstr> prog;
    std::vector<int32_t> obj_ranges;  // (first, count) per scene object
    std::vector<ProgTreeNode> prog_tree;  // nodes of every object's tree (instruction indices into prog)
    std::vector<int32_t> prog_roots;      // root node per scene object
    std::vector<RmPrim> prims;
    std::vector<float> world_pos; // Primitive.getWorldPosition() per primitive (BVH sort key)
    bool leaf_order = false;      // BVH sphere scenes: spheres / radii are stored in leaf order, bvh_prims is 0..n-1
    std::vector<int32_t> slot_object;  // with leaf_order: device slot -> object index (the sphere's place in the input list)
    std::vector<RmSphere> spheres;
    std::vector<double> radii;
    std::vector<float> prim_lo, prim_hi;  // padded AABBs, 3 floats per primitive
    std::vector<RmBvhNode> bvh;
    std::vector<int32_t> bvh_prims;
    int bvh_leaves = 0, bvh_depth = 0;
    // Uniform grid over the BVH root box that accelerates BVH.getPrimitivesAt (bvh.ts:95-121):
    // cell -> leaves whose box may contain a point of that cell (conservative), so the device
    // tests only those leaf boxes.  pq_cells[c] = (offset << 8) | count, count 255 = "walk the tree".
    int pq_dim[3] = {0, 0, 0};
    float pq_origin[3] = {0, 0, 0}, pq_inv[3] = {0, 0, 0};
    std::vector<uint32_t> pq_cells;
    std::vector<uint16_t> pq_list;
    // Same cells: spheres that can attain min_j Sphere.sdf for SOME point of the cell (the
    // all-primitive fallback of scene.ts:173 then only evaluates these).  count 255 = no list.
    int nn_dim[3] = {0, 0, 0};
    float nn_inv[3] = {0, 0, 0};
    std::vector<uint32_t> nn_cells;
    std::vector<uint16_t> nn_list;
    // The same lists for points OUTSIDE the root box (a ray that overshoots the scene: no leaf contains the point, scene.ts:173
    // evaluates every primitive): a coarse grid over the root box grown to where the orbit camera's rays can reach
    // (build_exterior_grid).  Same encoding; cells that lie inside the root box stay 255.  ext_dim[0] == 0: no grid.
    int ext_dim[3] = {0, 0, 0};
    float ext_origin[3] = {0, 0, 0}, ext_inv[3] = {0, 0, 0};
    std::vector<uint32_t> ext_cells;
    std::vector<uint16_t> ext_list;
    // Threshold tables of the leaf boxes, per axis (build_step_box; the v2 wave loop's in-round march steps test a new point
    // against the bracket of the round's point instead of against the leaf lists).  Axis k takes sb_stride words from word
    // k * sb_stride on: sb_bins look-up bytes, then the thresholds as binary32 bit patterns between -inf and +inf sentinels.
    // Empty: no table (no BVH sphere scene, more than kStepBoxCap thresholds on an axis, a tiny non-zero face coordinate).
    int sb_bins = 0, sb_stride = 0;
    float sb_origin[3] = {0, 0, 0}, sb_inv[3] = {0, 0, 0};
    std::vector<uint32_t> step_tab;
    // The threshold cells of step_tab as a table (build_cell_tab, sphere scenes only): per cell whether the root contains it, the
    // spheres of the leaves that contain it in scan order, their number, and a maximal block of cells with the same leaf set
    // (section B of the v2 wave loop reads its candidates there, section M its step box).  ct_dim: cells per axis; ct_rec_off /
    // ct_list_off: word offsets of the records and the sphere lists.  Empty: no table.
    int ct_dim[3] = {0, 0, 0};
    int ct_rec_off = 0, ct_list_off = 0;
    std::vector<uint32_t> cell_tab;
    std::vector<RmOctNode> oct;
    std::vector<int32_t> oct_prims;
    std::vector<RmSphereRec> oct_recs;  // oct_prims expanded to sphere records (sphere scenes)
    // Octree.findNode as one lookup: the tree is always the +-10 cube split at binary32 midpoints down to
    // depth 6 (scene.ts:81-85, octree.ts:60), so every leaf is a box of whole 0.3125-cells of a 64^3 grid
    // and every cell boundary -10 + 0.3125 k is exact in binary32.  oct_lut[(z*64 + y)*64 + x] = leaf node.
    std::vector<int32_t> oct_lut;
    // Crowded octree leaves (> 8 spheres): a grid of RM_OCT_SUB^3 sub-cells, each listing the positions (within the leaf's
    // list) of the spheres that can attain the leaf's minimum for SOME point of the sub-cell -- the same bound as the
    // BVH's nearest-candidate grid, but taken over the leaf's own list, which is what Scene.getDistance evaluates.
    std::vector<uint32_t> oct_sub_hdr;
    std::vector<uint8_t> oct_sub_list;
    bool prim_filter_ok = true;  // general scenes: every primitive's transform is rigid, `spheres` holds their bounding spheres
    int oct_leaves = 0, oct_empty = 0, oct_max_leaf = 0;
    float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};
};

// V8 Math.hypot for three arguments (used by boundingBox.ts:46,142-144)
double js_hypot3(double x, double y, double z);
// vec3.length / vec3.distance of the scene builder (box.ts:33, smoothUnion.ts:45): Math.hypot, or sqrt(x*x+y*y+z*z)
// after set_length_mode(1) (thread-local; the API layer sets it from the ctx before every build)
void set_length_mode(int use_sqrt);
double vec3_length_host(double x, double y, double z);

// sceneManager.ts:102-170: sphere-only presets 0..4; false for the others
bool preset_spheres(int index, std::vector<float> &centers, std::vector<double> &radii);

// The four pair loops of a sphere scene's build -- every (cell, sphere) or (node, box) pair, independent per cell or node --
// as they can be supplied from outside (rm_api.cpp: the device builder of rm_scene_build.hip).  Each member may be empty, and
// each call may return false: the host loop then builds that table, as it does without a PairLoops.  A supplier leaves the
// table as it found it when it returns false.  The trees, the leaf grid, the octree cell table and the leaf-order
// permutation (applied to nn_list / ext_list afterwards, whoever built them) stay with the host.
struct PairLoops {
    // build_point_query_grid, second half: nn_dim / nn_inv / pq_origin are set, nn_cells holds 255 per cell, nn_list is empty;
    // s.spheres / s.radii are in input order.  Fills nn_cells and nn_list.
    std::function<bool(HostScene &s)> nn_grid;
    // build_exterior_grid: ext_dim / ext_origin / ext_inv are set, ext_cells holds 255 per cell, ext_list is empty.
    std::function<bool(HostScene &s)> ext_grid;
    // The sub-cell lists of the crowded octree leaves `leaves` (node indices, increasing; sub_first and center are not set
    // yet): appends RM_OCT_SUB^3 headers per leaf to oct_sub_hdr and the lists to oct_sub_list, which are empty.  It must
    // refuse (false) when a leaf would start at or beyond 2^24 - RM_OCT_SUB^3 * prim_count entries: the host stops there.
    std::function<bool(HostScene &s, const std::vector<int32_t> &leaves)> oct_sub;
    // OctBuilder::nearest_prim_box (octree.ts:155-160) of the nodes `nodes`: out[i] = max(0, min over all primitive boxes of
    // box_gap(nodes[i], box)), 0 without a primitive.
    std::function<bool(const HostScene &s, const std::vector<int32_t> &nodes, std::vector<double> &out)> empty_dist;
};

// Builds spheres + acceleration structure.  Returns false and sets err on bad input.  `loops`: see PairLoops.
bool build_scene(HostScene &s, const float *centers, const double *radii, int n, int accel,
                 std::string &err, const PairLoops *loops = nullptr);

// SceneManager.getTransform (sceneManager.ts:21-37): world->local matrix of a primitive placed
// at (x, y, z); rot == nullptr is the branch without a rotation argument
void make_transform(double x, double y, double z, const float *rot, float out16[16]);

// presets 0-4 (spheres) and 5, 7, 8, 9 (torus / boxes) as primitive descriptions; false for
// presets that need SDF operators or the Mandelbulb
bool preset_prims(int index, std::vector<PrimDesc> &out);

// general scenes (any mix of spheres, boxes, tori, rotated or not)
bool build_scene_general(HostScene &s, const PrimDesc *prims, int n, int accel, std::string &err);

// presets 6 and 10-18 (SDF operators, Mandelbulb: sceneManager.ts:178-356) as expression forests
bool preset_nodes(int index, std::vector<NodeDesc> &nodes, std::vector<int> &roots);

// scenes whose objects are expression trees (any preset can be expressed this way)
bool build_scene_nodes(HostScene &s, const NodeDesc *nodes, int n_nodes, const int *roots, int n_roots, int accel,
                       std::string &err);

// A scene of plain primitives (spheres; spheres / boxes / tori with transforms) as one single-leaf expression object per
// primitive, in the scene's primitive order -- what the run-time specialiser (rm_rtc.h) needs to emit such a scene as code.
// False when the scene is an expression forest already, is empty, or holds a non-finite number.
bool leaf_objects(const HostScene &s, std::vector<RmInstr> &prog, std::vector<int32_t> &obj_ranges, std::vector<ProgTreeNode> &tree,
                  std::vector<int32_t> &roots);

// Option `exact` (include/rm_raymarch.h): the tree of boxes an exact query walks to find min over ALL objects of Primitive.sdf.
// Pruning a box needs sdf >= distance to the object's padded box for every object inside, which holds when Primitive.sdf is a
// true world-space distance to a body inside that box: sphere records, and primitive records whose transforms are all rigid
// (prim_filter_ok), with radii and extents that are finite and not negative.  exact_tree_mode says what such a query does:
//   0  every object is evaluated (expression forests, a non-rigid transform, a negative radius or extent, an empty scene, a
//      scene whose own tree could not be built: a leaf of more than 255 objects)
//   1  the scene's own BVH (s.bvh / s.bvh_prims)
//   2  an own tree (octree and None scenes): build_exact_tree
// The own tree is BvhBuilder's over s.prim_lo / prim_hi / world_pos -- skip-linked nodes in right-first pre-order and an id
// list; the ids index the scene's arrays as the scene's kernels index them (object order: only BVH sphere scenes are permuted)
// -- kept apart from the render tables of HostScene, which it does not touch.
struct ExactTree {
    std::vector<RmBvhNode> nodes;
    std::vector<int32_t> ids;
    int leaves = 0, depth = 0;
};
int exact_tree_mode(const HostScene &s);
// false (and an empty tree) when BvhBuilder refuses the scene; call only for mode 2
bool build_exact_tree(const HostScene &s, ExactTree &out);

// gl-matrix mat4.scale(m, m, [x, y, z]) in place (sceneManager.ts:63: the Mandelbulb's world->local is post-scaled)
void scale_transform(float m[16], double x, double y, double z);

// camera.ts:58-69,81-88 + raymarcher.ts:62-67
void camera_from_angles(double pitch, double yaw, float rot9[9], float origin3[3]);
// Math.min(Math.max(pitch, -Math.PI / 2), Math.PI / 2) (camera.ts:29,59) for a finite pitch
double clamp_pitch(double pitch);

// phongModel.ts:15-16
void phong_light_dir(float out[3]);

}  // namespace rmh
