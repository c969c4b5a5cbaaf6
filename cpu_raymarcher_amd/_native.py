"""Loader for the C-ABI library librm_hip.so (include/rm_raymarch.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded
this module raises, loudly.  `build()` compiles it in-tree with hipcc for gfx950.
"""
import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
# RM_HIP_LIB: another build of the same library (A/B measurements of two builds in one process each)
LIB_PATH = os.environ.get("RM_HIP_LIB") or os.path.join(_PKG, "librm_hip.so")
CSRC = os.path.join(_PKG, "csrc")

RM_OK = 0
RM_E_INVALID = -1
RM_E_UNSUPPORTED = -2
RM_E_NO_DEVICE = -3
RM_E_HIP = -4
RM_E_NO_SCENE = -5
RM_E_NOMEM = -6
RM_SCENE_UPLOADED = -(2 ** 31)

_STATUS_NAMES = {0: "RM_OK", -1: "RM_E_INVALID", -2: "RM_E_UNSUPPORTED", -3: "RM_E_NO_DEVICE",
                 -4: "RM_E_HIP", -5: "RM_E_NO_SCENE", -6: "RM_E_NOMEM"}


class RmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (_STATUS_NAMES.get(code, "?"), code, msg))
        self.code = code


class RmUnsupported(RmError):
    """RM_E_UNSUPPORTED: the host may fall back to its own CPU path."""


class rm_job(C.Structure):  # include/rm_raymarch.h: struct rm_job
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("time", C.c_double),
                ("y_start", C.c_int32), ("y_end", C.c_int32),
                ("camera_pitch", C.c_double), ("camera_yaw", C.c_double),
                ("algorithm", C.c_int32), ("scene_preset_index", C.c_int32),
                ("acceleration_structure", C.c_int32), ("reserved", C.c_int32),
                ("overshoot_factor", C.c_double), ("step_size", C.c_double)]


class rm_ray_query(C.Structure):  # include/rm_raymarch.h: struct rm_ray_query
    _fields_ = [("algorithm", C.c_int32), ("normal", C.c_int32), ("time", C.c_double),
                ("overshoot_factor", C.c_double), ("step_size", C.c_double)]


class rm_light(C.Structure):  # include/rm_raymarch.h: struct rm_light
    _fields_ = [("dir", C.c_float * 3), ("ao_samples", C.c_int32), ("bias", C.c_double), ("ao_step", C.c_double),
                ("ao_strength", C.c_double)]


class rm_step(C.Structure):  # include/rm_raymarch.h: struct rm_step
    _fields_ = [("t", C.c_double), ("value", C.c_double), ("count", C.c_uint32), ("kind", C.c_int32)]


class rm_walk(C.Structure):  # include/rm_raymarch.h: struct rm_walk
    _fields_ = [("t", C.c_double), ("min_dist", C.c_double), ("t_min", C.c_double), ("skipped", C.c_double),
                ("evals", C.c_uint32), ("skips", C.c_uint32), ("sdf_calls", C.c_uint32), ("end", C.c_int32)]


# the same two records as numpy structured dtypes (what Context.walk returns), rm_step_kind, rm_walk_end
STEP_DTYPE = [("t", "<f8"), ("value", "<f8"), ("count", "<u4"), ("kind", "<i4")]
WALK_DTYPE = [("t", "<f8"), ("min_dist", "<f8"), ("t_min", "<f8"), ("skipped", "<f8"), ("evals", "<u4"), ("skips", "<u4"),
              ("sdf_calls", "<u4"), ("end", "<i4")]
RM_STEP_EVAL, RM_STEP_SKIP = 0, 1
RM_END_HIT, RM_END_FAR, RM_END_STEPS, RM_END_ACCEL = 0, 1, 2, 3
WALK_ENDS = {0: "hit", 1: "far", 2: "steps", 3: "accel"}
RM_WALK_MAX_STEPS = 256


class rm_lattice(C.Structure):  # include/rm_raymarch.h: struct rm_lattice
    _fields_ = [("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("dw", C.c_float * 3),
                ("nu", C.c_int32), ("nv", C.c_int32), ("nw", C.c_int32), ("reserved", C.c_int32), ("time", C.c_double)]


class rm_field_shade(C.Structure):  # include/rm_raymarch.h: struct rm_field_shade
    _fields_ = [("map", C.c_int32), ("reserved", C.c_int32), ("range", C.c_double), ("band", C.c_double), ("line", C.c_double),
                ("lo", C.c_uint32), ("hi", C.c_uint32)]


# rm_field_map by name
FIELD_MAPS = {"distance": 0, "count": 1}


class rm_point_query(C.Structure):  # include/rm_raymarch.h: struct rm_point_query
    _fields_ = [("time", C.c_double), ("iso", C.c_double), ("snap_tol", C.c_double), ("snap_steps", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 2)]


RM_POINT_NORMAL = 1


class rm_sharp_query(C.Structure):  # include/rm_raymarch.h: struct rm_sharp_query
    _fields_ = [("iso", C.c_double), ("rank_tol", C.c_double), ("reach", C.c_double), ("refine", C.c_int32), ("reserved", C.c_int32)]


class rm_mesh_info(C.Structure):  # include/rm_raymarch.h: struct rm_mesh_info
    _fields_ = [("n_vertices", C.c_int64), ("n_quads", C.c_int64), ("n_holes", C.c_int64), ("reserved", C.c_int64)]


RM_MESH_F64, RM_MESH_F32 = 0, 1


class rm_sparse_info(C.Structure):  # include/rm_raymarch.h: struct rm_sparse_info
    _fields_ = [("n_blocks", C.c_int64), ("n_kept", C.c_int64), ("reserved", C.c_int64 * 2)]


RM_SPARSE_BLOCK = 8


class rm_measure(C.Structure):  # include/rm_raymarch.h: struct rm_measure
    _fields_ = [("n_points", C.c_int64), ("n_inside", C.c_int64), ("n_nonfinite", C.c_int64), ("sum1", C.c_int64 * 3), ("sum2", C.c_int64 * 6),
                ("crossings", C.c_int64 * 3), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("n_blocks", C.c_int64), ("n_kept", C.c_int64),
                ("n_blocks_inside", C.c_int64), ("reserved", C.c_int64)]


class rm_measure_world(C.Structure):  # include/rm_raymarch.h: struct rm_measure_world
    _fields_ = [("cell_volume", C.c_double), ("volume", C.c_double), ("centroid", C.c_double * 3), ("second", C.c_double * 6),
                ("projected_area", C.c_double * 3), ("area_estimate", C.c_double)]


class rm_parts_info(C.Structure):  # include/rm_raymarch.h: struct rm_parts_info
    _fields_ = [("n_points", C.c_int64), ("n_set", C.c_int64), ("n_parts", C.c_int64), ("gave_up", C.c_int64)]


RM_PARTS_INSIDE, RM_PARTS_OUTSIDE = 0, 1


class rm_edt_info(C.Structure):  # include/rm_raymarch.h: struct rm_edt_info
    _fields_ = [("n_points", C.c_int64), ("n_set", C.c_int64), ("max_d2", C.c_int64), ("argmax", C.c_int64)]


RM_EDT_FAR = 2 ** 31 - 1


class rm_view(C.Structure):  # include/rm_raymarch.h: struct rm_view
    _fields_ = [("camera_pitch", C.c_double), ("camera_yaw", C.c_double), ("time", C.c_double)]


class rm_frame_set(C.Structure):  # include/rm_raymarch.h: struct rm_frame_set
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("sdf", C.c_void_p), ("iters", C.c_void_p)]


class rm_compare_stats(C.Structure):  # include/rm_raymarch.h: struct rm_compare_stats
    _fields_ = [(name, C.c_uint64) for name in (
        "pixels", "sum_sdf_a", "sum_sdf_b", "sum_iters_a", "sum_iters_b", "sum_abs_depth", "surface_a", "surface_b",
        "surface_only_a", "surface_only_b", "depth_differs", "normal_differs", "counters_differ", "b_cheaper", "a_cheaper")] + \
        [("max_abs_depth", C.c_uint32), ("max_abs_normal", C.c_uint32)]


# rm_compare_map by name
COMPARE_MAPS = {"none": -1, "sdf": 0, "iters": 1, "depth": 2, "normal": 3, "surface": 4}

RM_HIST_BINS = 256


class rm_counter_hist(C.Structure):  # include/rm_raymarch.h: struct rm_counter_hist
    _fields_ = [("pixels", C.c_uint64), ("sum", C.c_uint64), ("min", C.c_uint32), ("max", C.c_uint32), ("range_lo", C.c_uint32),
                ("range_hi", C.c_uint32), ("shift", C.c_uint32), ("reserved", C.c_uint32), ("bins", C.c_uint32 * RM_HIST_BINS)]


class rm_frame_hist(C.Structure):  # include/rm_raymarch.h: struct rm_frame_hist
    _fields_ = [("sdf", rm_counter_hist), ("iters", rm_counter_hist)]


# rm_hist_mask by name
HIST_MASKS = {"all": 0, "surface": 1, "background": 2}


class rm_scene_info(C.Structure):
    _fields_ = [("n_prims", C.c_int32), ("accel", C.c_int32), ("preset_index", C.c_int32),
                ("bvh_nodes", C.c_int32), ("bvh_leaves", C.c_int32), ("bvh_depth", C.c_int32),
                ("oct_nodes", C.c_int32), ("oct_leaves", C.c_int32), ("oct_empty_leaves", C.c_int32),
                ("oct_max_leaf_prims", C.c_int32), ("root_min", C.c_float * 3), ("root_max", C.c_float * 3),
                ("nodes_in_lds", C.c_int32), ("program", C.c_int32)]


class rm_node(C.Structure):  # include/rm_raymarch.h: struct rm_node
    _fields_ = [("type", C.c_int32), ("child_a", C.c_int32), ("child_b", C.c_int32), ("reserved", C.c_int32),
                ("world_to_local", C.c_float * 16), ("params", C.c_double * 6)]


class rm_prim(C.Structure):  # include/rm_raymarch.h: struct rm_prim
    _fields_ = [("type", C.c_int32), ("reserved", C.c_int32), ("world_to_local", C.c_float * 16),
                ("params", C.c_double * 3), ("reserved2", C.c_double)]


class rm_sphere_edit(C.Structure):  # include/rm_raymarch.h: struct rm_sphere_edit
    _fields_ = [("op", C.c_int32), ("index", C.c_int32), ("center", C.c_float * 3), ("reserved", C.c_int32),
                ("radius", C.c_double)]


class rm_ball(C.Structure):  # include/rm_raymarch.h: struct rm_ball
    _fields_ = [("center", C.c_float * 3), ("reserved", C.c_int32), ("radius", C.c_double)]


class rm_tiles_update_info(C.Structure):  # include/rm_raymarch.h: struct rm_tiles_update_info
    _fields_ = [("n_kept", C.c_int64), ("n_reused", C.c_int64), ("n_evaluated", C.c_int64), ("reserved", C.c_int64)]


BALL_DTYPE = [("center", "<f4", (3,)), ("reserved", "<i4"), ("radius", "<f8")]  # rm_ball as a numpy record
RM_TILES_UPDATE_MAX_BALLS = 65536

# rm_edit_op by name, and the element type of every scene table rm_debug_scene_table names
RM_EDIT_SET, RM_EDIT_INSERT, RM_EDIT_REMOVE = 0, 1, 2
EDIT_OPS = {"set": 0, "insert": 1, "remove": 2}
SCENE_TABLES = {"spheres": "<f4", "radii": "<f8", "bvh": "u1", "bvh_prims": "<i4", "oct": "u1", "oct_prims": "<i4",
                "pq_cells": "<u4", "pq_list": "<u2", "nn_cells": "<u4", "nn_list": "<u2", "prims": "u1", "prog": "u1",
                "obj_ranges": "<i4", "oct_recs": "u1", "oct_lut": "<i4", "oct_sub_hdr": "<u4", "oct_sub_list": "u1",
                "slot_object": "<i4", "ext_cells": "<u4", "ext_list": "<u2", "step_tab": "<u4", "cell_tab": "<u4"}
# step_tab (csrc/rm_scene_host.h): look-up bins per axis, one byte each, ahead of the thresholds; thresholds an axis may hold
STEP_BOX_BINS, STEP_BOX_CAP = 32, 62


class rm_diagnostics(C.Structure):
    _fields_ = [("total_sdf_calls", C.c_uint64), ("total_iterations", C.c_uint64),
                ("max_sdf_calls", C.c_uint32), ("min_sdf_calls", C.c_uint32), ("total_pixels", C.c_uint64)]


# every symbol include/rm_raymarch.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
SIGNATURES = {
    "rm_create": (C.c_int, [C.c_int, C.POINTER(_VP)]),
    "rm_destroy": (None, [_VP]),
    "rm_last_error": (C.c_char_p, [_VP]),
    "rm_last_kernel": (C.c_char_p, [_VP]),
    "rm_version": (C.c_char_p, []),
    "rm_algorithm_from_string": (C.c_int, [C.c_char_p]),
    "rm_accel_from_string": (C.c_int, [C.c_char_p]),
    "rm_shader_from_string": (C.c_int, [C.c_char_p]),
    "rm_preset_count": (C.c_int, []),
    "rm_scene_from_preset": (C.c_int, [_VP, C.c_int32, C.c_int32]),
    "rm_scene_from_spheres": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32]),
    "rm_scene_edit_spheres": (C.c_int, [_VP, C.POINTER(rm_sphere_edit), C.c_int32]),
    "rm_debug_scene_table": (C.c_int, [_VP, C.c_char_p, C.c_int32, _VP, C.c_int64, C.POINTER(C.c_int64)]),
    "rm_selftest_hypot64": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, _VP]),
    "rm_scene_from_prims": (C.c_int, [_VP, C.POINTER(rm_prim), C.c_int32, C.c_int32]),
    "rm_make_transform": (C.c_int, [C.c_double, C.c_double, C.c_double, _VP, _VP]),
    "rm_scene_from_nodes": (C.c_int, [_VP, C.POINTER(rm_node), C.c_int32, _VP, C.c_int32, C.c_int32]),
    "rm_scale_transform": (C.c_int, [_VP, C.c_double, C.c_double, C.c_double]),
    "rm_scene_set_time": (C.c_int, [_VP, C.c_double]),
    "rm_selftest_jsmath": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int64, _VP]),
    "rm_scene_get_info": (C.c_int, [_VP, C.POINTER(rm_scene_info)]),
    "rm_camera_from_angles": (C.c_int, [C.c_double, C.c_double, _VP, _VP]),
    "rm_scene_distance": (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP]),
    "rm_debug_wave_distance": (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP]),
    "rm_scene_field": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, _VP, _VP]),
    "rm_scene_field_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, _VP, _VP, _VP]),
    "rm_scene_points": (C.c_int, [_VP, C.POINTER(rm_point_query), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_scene_points_device": (C.c_int, [_VP, C.POINTER(rm_point_query), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_lattice_points": (C.c_int, [C.POINTER(rm_lattice), C.c_int64, C.c_int64, _VP]),
    "rm_shade_field_device": (C.c_int, [_VP, C.POINTER(rm_field_shade), C.c_int64, _VP, _VP, _VP]),
    "rm_shade_field": (C.c_int, [_VP, C.POINTER(rm_field_shade), C.c_int64, _VP, _VP]),
    "rm_mesh_field_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, C.c_int32, C.c_double, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP]),
    "rm_scene_mesh": (C.c_int, [_VP, C.POINTER(rm_lattice), C.c_double, _VP, C.c_int64, _VP, C.c_int64, C.POINTER(rm_mesh_info)]),
    "rm_mesh_cells_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, C.c_int32, C.c_double, _VP, C.c_int64, _VP, _VP]),
    "rm_scene_sharpen_device": (C.c_int, [_VP, C.POINTER(rm_lattice), C.POINTER(rm_sharp_query), C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "rm_scene_sharpen": (C.c_int, [_VP, C.POINTER(rm_lattice), C.POINTER(rm_sharp_query), C.c_int64, _VP, _VP, _VP, _VP]),
    "rm_lattice_blocks": (C.c_int, [C.POINTER(rm_lattice), C.POINTER(C.c_int32)]),
    "rm_scene_blocks_device": (C.c_int, [_VP, C.POINTER(rm_lattice), C.c_double, C.c_double, _VP, _VP, _VP, _VP, _VP]),
    "rm_scene_tiles_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, C.c_int64, _VP, _VP]),
    "rm_scene_edit_balls": (C.c_int, [_VP, C.POINTER(rm_sphere_edit), C.c_int32, C.POINTER(rm_ball), C.c_int32, C.POINTER(C.c_int32)]),
    "rm_scene_tiles_update_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, _VP, C.c_int64, _VP, C.c_int32, _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "rm_mesh_tiles_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, _VP, C.c_int64, _VP, C.c_double, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP,
                                       _VP, _VP]),
    "rm_scene_mesh_sparse": (C.c_int, [_VP, C.POINTER(rm_lattice), C.c_double, C.c_double, _VP, C.c_int64, _VP, C.c_int64, _VP, _VP,
                                       C.POINTER(rm_mesh_info), C.POINTER(rm_sparse_info)]),
    "rm_measure_field_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, C.c_int32, C.c_double, _VP, _VP]),
    "rm_measure_tiles_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, _VP, C.c_int64, _VP, _VP, C.c_double, _VP, _VP]),
    "rm_scene_measure": (C.c_int, [_VP, C.POINTER(rm_lattice), C.c_double, C.c_double, C.POINTER(rm_measure), C.POINTER(rm_sparse_info)]),
    "rm_measure_world": (C.c_int, [C.POINTER(rm_lattice), C.POINTER(rm_measure), C.POINTER(rm_measure_world)]),
    "rm_label_field_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, C.c_int32, C.c_double, C.c_int32, _VP, _VP, _VP]),
    "rm_measure_labels_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, C.c_int64, _VP, _VP]),
    "rm_scene_parts": (C.c_int, [_VP, C.POINTER(rm_lattice), C.c_double, C.c_int32, _VP, C.c_int64, _VP, C.POINTER(rm_parts_info)]),
    "rm_edt_field_device": (C.c_int, [_VP, C.POINTER(rm_lattice), _VP, C.c_int32, C.c_double, C.c_int32, _VP, _VP, _VP]),
    "rm_scene_edt": (C.c_int, [_VP, C.POINTER(rm_lattice), C.c_double, C.c_int32, _VP, C.POINTER(rm_edt_info)]),
    "rm_lattice_cubic": (C.c_int, [C.POINTER(rm_lattice), C.POINTER(C.c_double)]),
    "rm_ray_march": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_ray_march_device": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_camera_rays": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, _VP, _VP]),
    "rm_ray_pick": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_ray_pick_device": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_ray_light": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.POINTER(rm_light), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                               _VP]),
    "rm_ray_light_device": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.POINTER(rm_light), C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                      _VP, _VP, _VP]),
    "rm_ray_walk": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.c_int64, _VP, _VP, C.c_int32, _VP, _VP]),
    "rm_ray_walk_device": (C.c_int, [_VP, C.POINTER(rm_ray_query), C.c_int64, _VP, _VP, C.c_int32, _VP, _VP, _VP]),
    "rm_phong_light": (C.c_int, [_VP]),
    "rm_shade_lit_device": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_shade_lit": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    "rm_scene_object": (C.c_int, [_VP, C.c_int32, C.POINTER(rm_node), C.c_int32, C.POINTER(C.c_int32)]),
    "rm_render_tile": (C.c_int, [_VP, C.POINTER(rm_job), _VP, _VP, _VP, _VP]),
    "rm_render_tile_device": (C.c_int, [_VP, C.POINTER(rm_job), C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_render_frames_device": (C.c_int, [_VP, C.POINTER(rm_job), C.c_int32, _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_compare_frames_device": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(rm_frame_set), C.POINTER(rm_frame_set),
                                           C.c_int32, C.c_int32, _VP, _VP, _VP]),
    "rm_compare_frames": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.POINTER(rm_frame_set), C.POINTER(rm_frame_set),
                                    C.c_int32, C.c_int32, _VP, _VP]),
    "rm_counter_hist_device": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         _VP, _VP]),
    "rm_counter_hist": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP]),
    "rm_shade_ranged_device": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_uint32, C.c_uint32, _VP, _VP]),
    "rm_shade_ranged": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, C.c_uint32, C.c_uint32, _VP]),
    "rm_sweep_views": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, _VP]),
    "rm_render_stripes_device": (C.c_int, [_VP, C.POINTER(rm_job), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_stripe_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rm_deal_stripes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _VP, _VP]),
    "rm_render_stripe_list_device": (C.c_int, [_VP, C.POINTER(rm_job), C.c_int32, C.c_int32, _VP, C.c_int32,
                                               _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_assemble_frame_device": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _VP,
                                           C.c_int32, C.c_int32, _VP, C.c_int64, _VP, _VP]),
    "rm_shade": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    "rm_shade_device": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_reduce_counters": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.POINTER(rm_diagnostics)]),
    "rm_reduce_counters_device": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.POINTER(rm_diagnostics), _VP]),
    "rm_reduce_counters_enqueue": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP]),
    "rm_render_attach_diagnostics": (C.c_int, [_VP, _VP]),
    "rm_partition_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rm_selftest_hypot": (C.c_int, [_VP, _VP, C.c_int64, _VP]),
    "rm_selftest_fastdiv": (C.c_int, [_VP, C.c_uint64, C.c_int64, C.POINTER(C.c_uint64)]),
    "rm_selftest_recip": (C.c_int, [_VP, C.c_int, _VP]),
    "rm_debug_read_stamps": (C.c_int, [_VP, _VP]),
    "rm_debug_read_wave_times": (C.c_int, [_VP, _VP]),
    "rm_debug_read_batch_log": (C.c_int, [_VP, _VP]),
    "rm_debug_read_counts": (C.c_int, [_VP, _VP]),
    "rm_debug_read_lpt_costs": (C.c_int, [_VP, _VP, C.c_int64]),
    "rm_debug_launch_fill": (C.c_int, [_VP, C.c_int32, C.POINTER(C.c_int32)]),
    "rm_debug_last_launch": (C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    "rm_debug_overlap_fill": (C.c_int, [_VP, C.c_int32, C.c_int64, C.POINTER(C.c_int32)]),
    "rm_debug_step_box": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "rm_debug_cell_tab": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "rm_debug_runner_up": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "rm_debug_scan_keys": (C.c_int, [_VP, C.c_int64, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "rm_debug_exact_tree": (C.c_int, [_VP, C.POINTER(C.c_int32)]),
    "rm_debug_rect_cull": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "rm_debug_leaf_rects": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP, C.c_int64, C.POINTER(C.c_int64)]),
    "rm_rtc_source": (C.c_int, [_VP, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "rm_rtc_compile_check": (C.c_int, [_VP, C.c_int32, C.c_int32, C.c_char_p, C.c_int64, C.POINTER(C.c_double)]),
    "rm_rtc_status": (C.c_int, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int64]),
    "rm_set_option": (C.c_int, [_VP, C.c_char_p, C.c_int64]),
    "rm_get_option": (C.c_int, [_VP, C.c_char_p, C.POINTER(C.c_int64)]),
}

_lib = None


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 ... -> cpu_raymarcher_amd/librm_hip.so (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h"))]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "rm_raymarch.h"))
    if not force and os.path.exists(LIB_PATH) and all(
            os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    cmd = ["make", "-j%d" % min(8, os.cpu_count() or 1), "-C", CSRC, "all"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def lib():
    """The loaded library; raises if it is absent (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "cpu_raymarcher_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C cpu_raymarcher_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7, and a
        # second runtime opened later finds no GPU ("No HIP GPUs are available").  Loading
        # torch first makes librm_hip.so's NEEDED libamdhip64.so.7 resolve to that copy.
        # Pure C / N-API consumers (no torch) get /opt/rocm's runtime through RUNPATH.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("RM_HIP_LIB") and not hasattr(L, name):
                continue  # A/B measurements against an OLDER build of the library (scripts/kbench.py): newer entry points are absent there
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(ctx, rc):
    if rc == RM_OK:
        return
    msg = lib().rm_last_error(ctx).decode() if ctx else ""
    raise (RmUnsupported if rc == RM_E_UNSUPPORTED else RmError)(rc, msg)
