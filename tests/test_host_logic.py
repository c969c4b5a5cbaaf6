"""CPU tests of the product's host side: the C-ABI library loads and exports every symbol
include/rm_raymarch.h declares, and the host logic (presets, camera, BVH/Octree build,
partition, string defaulting, error codes) agrees with the oracle.  No compute calls."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(rm):
    from cpu_raymarcher_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "rm_raymarch.h")).read()
    declared = set(re.findall(r"RM_API\s+[\w\s\*]+?\b(rm_\w+)\s*\(", hdr))
    assert len(declared) >= 20
    assert declared == set(N.SIGNATURES), declared ^ set(N.SIGNATURES)
    lib = C.CDLL(N.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in N.lib().rm_version()


def test_struct_layouts_match_header(rm):
    from cpu_raymarcher_amd import _native as N
    assert C.sizeof(N.rm_job) == 72 and N.rm_job.camera_pitch.offset == 24 and N.rm_job.step_size.offset == 64
    assert C.sizeof(N.rm_scene_info) == 72
    assert C.sizeof(N.rm_diagnostics) == 32
    assert C.sizeof(N.rm_node) == 128 and N.rm_node.params.offset == 80 and C.sizeof(N.rm_prim) == 104


def test_string_defaulting_rules(rm):
    from cpu_raymarcher_amd import _native as N
    L = N.lib()
    # raymarchWorker.ts:50-68: unknown -> sphere tracer
    assert [L.rm_algorithm_from_string(s.encode()) for s in
            ("sphere-tracer", "fixed-step", "adaptive-step", "adaptive-step-v2", "adaptive-step-v3", "bogus", "")] == \
        [0, 1, 2, 3, 4, 0, 0]
    # scene.ts:32-36: anything else -> None (case-sensitive)
    assert [L.rm_accel_from_string(s.encode()) for s in ("None", "Octree", "BVH", "bvh", "")] == [0, 1, 2, 0, 0]
    # main.ts:33-45
    assert [L.rm_shader_from_string(s.encode()) for s in ("normal", "phong", "sdf-heatmap", "iteration-heatmap", "x")] \
        == [0, 1, 2, 3, 0]
    assert L.rm_preset_count() == 19


def test_partition_rows_matches_main_ts(rm):
    # main.ts:444-449: r = ceil(H / N); [min(i r, H), min((i+1) r, H))
    for H in (1, 7, 128, 1080, 2160):
        for n in (1, 2, 3, 4, 7, 8, 16):
            r = math.ceil(H / n)
            rows = [rm.partition_rows(H, n, i) for i in range(n)]
            assert rows == [(min(i * r, H), min((i + 1) * r, H)) for i in range(n)]
            assert sum(b - a for a, b in rows) == H


def test_host_only_context_builds_scenes_like_the_oracle(rm, oracle):
    ctx = rm.Context(None)
    for preset in range(19):  # 6 and 10-18: operator trees / Mandelbulb (bounds from the overridden getters)
        for accel, name in ((0, "None"), (1, "Octree"), (2, "BVH")):
            ctx.scene_from_preset(preset, accel)
            info = ctx.scene_info()
            osc = oracle.OracleScene(preset=preset, accel=name)
            st = osc.stats()
            assert info["n_prims"] == st["n"]
            assert (info["bvh_nodes"], info["bvh_leaves"], info["bvh_depth"]) == \
                (st["bvh_nodes"], st["bvh_leaves"], st["bvh_depth"])
            assert (info["oct_nodes"], info["oct_leaves"], info["oct_empty_leaves"], info["oct_max_leaf_prims"]) == \
                (st["oct_nodes"], st["oct_leaves"], st["oct_empty"], st["oct_maxleafprims"])
            rb = osc.root_bounds()
            if rb is not None:
                assert np.array_equal(np.float32(info["root_min"] + info["root_max"]), rb)
    sp = oracle.synthetic_spheres(3000)
    for accel, name in ((1, "Octree"), (2, "BVH")):
        ctx.scene_from_spheres(sp[:, :3], sp[:, 3], accel)
        info = ctx.scene_info()
        st = oracle.OracleScene(spheres=sp, accel=name).stats()
        assert (info["bvh_nodes"], info["bvh_leaves"], info["bvh_depth"], info["oct_nodes"], info["oct_leaves"],
                info["oct_empty_leaves"], info["oct_max_leaf_prims"]) == \
            (st["bvh_nodes"], st["bvh_leaves"], st["bvh_depth"], st["oct_nodes"], st["oct_leaves"], st["oct_empty"],
             st["oct_maxleafprims"])


def test_camera_matches_oracle(rm, oracle):
    sc = oracle.OracleScene(preset=0, accel="None")
    rng = np.random.default_rng(3)
    for pitch, yaw in [(0, 0), (0.3, 0.7), (-2.0, 9.0), (math.pi / 2, -math.pi)] + list(rng.uniform(-4, 4, (200, 2))):
        sc.set_angles(pitch, yaw)
        rot, org = sc.camera()
        r2, o2 = rm.camera_from_angles(pitch, yaw)
        assert np.array_equal(rot, r2) and np.array_equal(org, o2)


def test_error_codes_without_a_device(rm):
    from cpu_raymarcher_amd import _native as N
    ctx = rm.Context(None)
    ctx.scene_from_preset(99, 2)  # scene.ts:39 clamps to preset 18 ("67")
    assert ctx.scene_info()["n_prims"] == 2
    ident = np.eye(4, dtype=np.float32).ravel()
    moved = ident.copy()
    moved[12] = 0.25  # a Round takes its operand's transform (round.ts): translated, every level needs a position slot of its own
    chain = [(0, -1, -1, moved, [0.5])] + [(10, i, -1, None, [0.01]) for i in range(20)]  # 20 nested Round operators
    with pytest.raises(rm.RmUnsupported):
        ctx.scene_from_nodes(chain, [len(chain) - 1], 0)
    ctx.scene_from_nodes(chain[:10], [9], 2)
    assert ctx.scene_info()["n_prims"] == 1
    ctx.scene_from_nodes([(0, -1, -1, ident, [0.5])] + [(10, i, -1, None, [0.01]) for i in range(20)], [20], 0)  # identity transforms pass the point through: no slot per level
    assert ctx.scene_info()["n_prims"] == 1
    with pytest.raises(rm.RmError):  # operands must precede their operator
        ctx.scene_from_nodes([(10, 1, -1, None, [0.1]), (0, -1, -1, ident, [0.5])], [0], 0)
    with pytest.raises(rm.RmError):
        ctx.scene_from_nodes([(42, -1, -1, ident, [0.5])], [0], 0)
    ctx.scene_from_preset(-5, 2)  # clamps to preset 0
    assert ctx.scene_info()["n_prims"] == 1
    scene = rm.Scene("BVH", ctx=ctx)
    scene.loadPreset(3)
    buf = [np.zeros(16, np.uint8), np.zeros(48, np.uint8), np.zeros(16, np.uint16), np.zeros(16, np.uint16)]
    with pytest.raises(rm.RmError) as e:  # there is no CPU render path
        rm.SphereTracer().runRaymarcher(scene, *buf, 4, 4)
    assert e.value.code == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError):
        ctx.scene_from_spheres(np.array([[0, 0, float("nan")]]), np.array([1.0]), 0)
    with pytest.raises(rm.RmError):
        ctx.set_option("tile_w", 12)
    ctx.set_option("tile_w", 16)
    assert ctx.get_option("tile_w") == 16
    # the round-2 knobs: defaults, accepted values, rejected values, unknown keys
    assert (ctx.get_option("oct_lean"), ctx.get_option("v1_block"), ctx.get_option("v1_lists"), ctx.get_option("lpt")) == (1, 64, 1, 1)
    # the round-3 knobs
    assert (ctx.get_option("multi_step"), ctx.get_option("blocks_per_cu"), ctx.get_option("lds_kb"), ctx.get_option("lds_fill")) == (1, 6, 0, 0)
    ctx.set_option("static", 75)  # accepted, ignored since round 3
    for bad in (8, 65):
        with pytest.raises(rm.RmError):
            ctx.set_option("lds_kb", bad)
    for bad in (0, 32, 96, 512):
        with pytest.raises(rm.RmError):
            ctx.set_option("v1_block", bad)
    for good in (128, 256, 64):
        ctx.set_option("v1_block", good)
        assert ctx.get_option("v1_block") == good
    ctx.set_option("oct_lean", 0)
    assert ctx.get_option("oct_lean") == 0
    ctx.set_option("oct_lean", 7)  # any non-zero value switches it on
    assert ctx.get_option("oct_lean") == 1
    with pytest.raises(rm.RmError):
        ctx.set_option("no_such_option", 1)
    with pytest.raises(rm.RmError):
        ctx.get_option("no_such_option")


def test_camera_class_mirrors_reference(rm):
    cam = rm.Camera()
    cam.setAngles(9.0, 1.0)
    assert cam.getAngles() == [math.pi / 2, 1.0]
    cam.rotateCamera(-0.5, 0.015)
    assert cam.getAngles() == [math.pi / 2 - 0.5, 1.015]
    assert isinstance(rm.createRaymarcher("nope"), rm.SphereTracer)
    assert isinstance(rm.createRaymarcher("fixed-step", stepSize=0.1), rm.FixedStep)
    assert isinstance(rm.createShadingModelFromValue("nope"), rm.NormalModel)
    assert isinstance(rm.createShadingModelFromValue("phong"), rm.PhongModel)


def test_synthetic_scene_definitions_agree_with_the_oracles_copy(rm, oracle):
    from cpu_raymarcher_amd import synthetic as S
    assert np.array_equal(S.synthetic_spheres(500), oracle.synthetic_spheres(500))
    assert S.synthetic_mixed_prims(30, seed=11) == oracle.synthetic_mixed_prims(30, seed=11)
    triples = S.mixed_prims_as_triples(S.synthetic_mixed_prims(12), rm.make_transform)
    want = oracle.OracleScene(accel="None", prims=oracle.synthetic_mixed_prims(12)).prims()
    for (t, m, par), (wt, wm, wpar) in zip(triples, want):
        assert t == wt and np.array_equal(m, wm) and list(par) == list(wpar[:len(par)])


def _switch(default):  # 0 | 1: any non-zero value is 1
    return dict(default=default, accepted=[(0, 0), (1, 1), (7, 1), (-1, 1), (0, 0)], rejected=[])


def _range(default, lo, hi):  # inclusive range
    return dict(default=default, accepted=[(lo, lo), (hi, hi), ((lo + hi) // 2, (lo + hi) // 2)], rejected=[lo - 1, hi + 1, -(1 << 40), 1 << 40])


def _set(default, values, between):  # a short explicit value set
    return dict(default=default, accepted=[(v, v) for v in values], rejected=[min(values) - 1, max(values) + 1, 0, -min(values)] + between)


# one row per key of include/rm_raymarch.h's option list: default, (probe, value stored) pairs, rejected probes
OPTION_CONTRACT = {
    "tile_w": _set(8, [8, 16, 32, 64], [12, 24, 48]),
    "filter": _switch(1),
    "nodes_in_lds": _switch(1),
    "kernel": _range(0, 0, 2),
    "list_cap": _range(32, 1, 64),
    "coop": _switch(1),
    "grid": _switch(1),
    "nn": _range(2, 0, 2),
    "recs": _switch(1),
    "lut": _switch(1),
    "sub": _switch(1),
    "blocks_per_cu": _range(6, 1, 8),
    "refill": _range(64, 1, 64),
    "hw_xcd": _switch(1),
    "item_px": _set(128, [64, 128, 256], [96, 192]),
    "static": _range(0, 0, 95),  # accepted, stored, ignored
    "uniform": _switch(1),
    "rel": _switch(1),
    "cull": _switch(1),
    "lds_kb": dict(default=0, accepted=[(16, 16), (64, 64), (32, 32), (0, 0), (40, 40)], rejected=[-1, 1, 8, 15, 65, 1 << 40]),  # 0 or a range
    "n0_batch": _range(64, 1, 64),
    "lpt": _switch(1),
    "multi_step": _switch(1),
    "lds_fill": _switch(0),
    "item_wide": _switch(0),
    "specialise": _range(1, 0, 2),
    "specialise_v2_after": _range(3, 0, 1000000),
    "rtc_spheres": _range(16, 0, 33),
    "prune": _switch(1),
    "v1_lists": _switch(1),
    "v1_block": _set(64, [64, 128, 256], [96, 192]),
    "oct_lean": _switch(1),
    "length": dict(default=0, accepted=[(1, 1), (0, 0)], rejected=[-1, 2, 7]),  # strictly 0 or 1: part of the numeric contract
}


def test_every_option_keeps_its_contract(rm):
    """Every key of rm_set_option / rm_get_option (include/rm_raymarch.h lists 33): its default, the values it takes and
    how they are stored, the values it refuses -- those just outside every range and between the members of every set --
    which leave the stored value alone and an error text behind; unknown keys fail both ways."""
    from cpu_raymarcher_amd import _native as N
    assert len(OPTION_CONTRACT) == 33
    ctx = rm.Context(None)
    last = {key: row["default"] for key, row in OPTION_CONTRACT.items()}
    assert {key: ctx.get_option(key) for key in OPTION_CONTRACT} == last
    for key, row in OPTION_CONTRACT.items():
        for probe, stored in row["accepted"]:
            ctx.set_option(key, probe)
            assert ctx.get_option(key) == stored, (key, probe)
            for bad in row["rejected"]:
                with pytest.raises(rm.RmError) as e:
                    ctx.set_option(key, bad)
                assert e.value.code == N.RM_E_INVALID, (key, bad)
                assert N.lib().rm_last_error(ctx._h).decode() != "", (key, bad)
                assert ctx.get_option(key) == stored, (key, bad)
        last[key] = row["accepted"][-1][1]
        assert {k: ctx.get_option(k) for k in OPTION_CONTRACT} == last, key  # no key writes another's value
    for key in ("", "no_such_option", "tile_w ", "Tile_w", "opt_tile_w"):
        with pytest.raises(rm.RmError):
            ctx.set_option(key, 1)
        with pytest.raises(rm.RmError):
            ctx.get_option(key)
    ctx.close()
    # `length` rebuilds the active scene (no device needed): with no scene, with a preset, after a sphere upload
    ctx = rm.Context(None)
    for scene in (None, "preset", "spheres"):
        if scene == "preset":
            ctx.scene_from_preset(9, 2)
        elif scene == "spheres":
            ctx.scene_from_spheres(np.float32([[0, 0, 0], [1, 0.5, 0], [0, 1, 0.25]]), [0.5, 0.25, 0.125], 1)
        before = ctx.scene_info() if scene else None
        for v in (1, 1, 0, 0):
            ctx.set_option("length", v)
            assert ctx.get_option("length") == v
            if scene:
                assert ctx.scene_info() == before, (scene, v)  # same scene, same structure: the two forms differ by an ulp
                assert len(ctx.scene_object(0)) == 1
    ctx.close()


def test_uploads_of_every_kind_replace_one_another(rm):
    """rm_scene_from_spheres / _prims / _nodes keep one description of the upload: each call replaces the one before,
    whatever its kind (rm_scene_object reads it back), a refused upload replaces nothing, and the remembered upload is
    what a rebuild builds from (the `length` option rebuilds the active scene)."""
    ctx = rm.Context(None)
    ident = np.eye(4, dtype=np.float32).ravel()
    centers, radii = np.float32([[0.5, 0, 0], [0, 0.25, 0], [0, 0, -0.75]]), [0.5, 0.25, 0.125]
    box = rm.make_transform(0.25, -0.5, 0.125, [0.1, 0.2, 0.3])
    prims = [(1, box, [0.5, 0.25, 0.125]), (2, ident, [0.5, 0.125])]
    nodes = [(0, -1, -1, rm.make_transform(0.25, 0, 0), [0.5]), (1, -1, -1, ident, [0.25, 0.5, 0.125]), (11, 0, 1, None, [0.0625])]

    def sphere_0(c, r):
        (t, a, b, m, par), = ctx.scene_object(0)
        assert (t, a, b) == (0, -1, -1) and np.array_equal(m, rm.make_transform(*[float(v) for v in c])) and par[0] == r

    def prim_0():
        (t, a, b, m, par), = ctx.scene_object(0)
        assert (t, a, b) == (1, -1, -1) and np.array_equal(m, box) and list(par[:3]) == [0.5, 0.25, 0.125]

    def forest_0():
        got = ctx.scene_object(0)
        assert [(t, a, b) for t, a, b, _, _ in got] == [(0, -1, -1), (1, -1, -1), (11, 0, 1)]
        assert np.array_equal(got[0][3], nodes[0][3]) and got[0][4][0] == 0.5 and got[2][4][0] == 0.0625

    def rebuilt(check):  # the active scene built again from the remembered upload
        for v in (1, 0):
            ctx.set_option("length", v)
            check()

    ctx.scene_from_spheres(centers, radii, 2)
    assert ctx.scene_info()["n_prims"] == 3
    sphere_0(centers[0], 0.5)
    ctx.scene_from_prims(prims, 2)
    assert ctx.scene_info()["n_prims"] == 2
    prim_0()
    rebuilt(prim_0)
    ctx.scene_from_nodes(nodes, [2], 1)
    assert ctx.scene_info()["n_prims"] == 1 and ctx.scene_info()["prog_instructions"] > 0
    forest_0()
    # refused uploads of every kind: the forest stays the active scene and the remembered upload
    with pytest.raises(rm.RmError):
        ctx.scene_from_spheres(np.float32([[0, float("nan"), 0]]), [1.0], 1)
    with pytest.raises(rm.RmError):
        ctx.scene_from_prims([(7, ident, [0.5])], 1)
    with pytest.raises(rm.RmError):
        ctx.scene_from_nodes([(42, -1, -1, ident, [0.5])], [0], 1)
    assert ctx.scene_info()["n_prims"] == 1
    forest_0()
    rebuilt(forest_0)
    assert ctx.scene_info()["prog_instructions"] > 0
    ctx.scene_from_spheres(centers[1:], radii[1:], 0)
    assert ctx.scene_info()["n_prims"] == 2 and ctx.scene_info()["prog_instructions"] == 0
    sphere_0(centers[1], 0.25)
    rebuilt(lambda: sphere_0(centers[1], 0.25))
    ctx.scene_from_preset(3, 2)  # a preset in between does not forget the upload ...
    assert ctx.scene_info()["n_prims"] > 2 and len(ctx.scene_object(0)) == 1
    ctx.scene_from_prims(prims, 0)
    prim_0()
    ctx.close()


def test_device_entries_keep_their_order_of_refusals(rm):
    """Every exported entry that needs a device, called through ctypes (no Python-side validation in the way): the code of
    a null context; the code and rm_last_error text of a host-only context with otherwise valid arguments; and which
    refusal wins when one argument is bad as well.  The order of the checks and the texts are behaviour: some entries
    look at an argument before the device (the accumulator of rm_reduce_counters_enqueue, the query, count and buffers of
    a ray query), the others at the device first.  Every call is refused before any copy, so no pointer is dereferenced."""
    from cpu_raymarcher_amd import _native as N
    L = N.lib()
    ctx = rm.Context(None)
    ctx.scene_from_preset(0, 0)
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    odd = buf[1:].ctypes.data_as(C.c_void_p)  # inside the same buffer, not 8-byte aligned
    ids = np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)
    job = N.rm_job(width=4, height=4, y_end=4)
    J, Q = C.byref(job), C.byref(N.rm_ray_query())
    D, U = C.byref(N.rm_diagnostics()), C.byref(C.c_uint64(0))
    INVALID, NO_DEVICE = N.RM_E_INVALID, N.RM_E_NO_DEVICE
    HOST, RENDER, RAY = "host-only context", "host-only context: there is no CPU render path", "host-only context: there is no CPU ray path"
    KEPT = "unknown option no_such_option"  # the text a refused rm_set_option leaves before every call: the entry set none
    five = (p, p, p, p, p)

    def rays(device, pick):  # rm_ray_march / _device, rm_ray_pick / _device: the arguments behind (query, n, origins, dirs)
        tail = (p, p, p, p) + ((p,) if pick else ()) + ((None,) if device else ())
        return ((Q, 2, p, p) + tail, RAY,
                [((None, 2, p, p) + tail, INVALID, "null query"), ((Q, -1, p, p) + tail, INVALID, "ray count out of range"),
                 ((Q, 1 << 31, p, p) + tail, INVALID, "ray count out of range"), ((Q, 2, None, p) + tail, INVALID, "null ray buffer"),
                 ((Q, 2, p, None) + tail, INVALID, "null ray buffer"), ((None, -1, None, None) + tail, INVALID, "null query")])

    # entry: (valid arguments behind the context, text of the host-only refusal, [(arguments with one bad, code, text)])
    table = {
        "rm_render_tile_device": ((J, 0) + five + (None,), RENDER, [((None, 0) + five + (None,), NO_DEVICE, RENDER)]),
        "rm_render_stripes_device": ((J, 0, 16, 2, 0) + five + (None,), RENDER,
                                     [((None, 0, 16, 2, 0) + five + (None,), NO_DEVICE, RENDER), ((J, 0, 16, 0, 0) + five + (None,), NO_DEVICE, RENDER)]),
        "rm_render_stripe_list_device": ((J, 0, 16, ids, 1) + five + (None,), RENDER,
                                         [((None, 0, 16, ids, 1) + five + (None,), NO_DEVICE, RENDER), ((J, 0, 0, None, 1) + five + (None,), NO_DEVICE, RENDER)]),
        "rm_render_tile": ((J, p, p, p, p), RENDER, [((None, p, p, p, p), NO_DEVICE, RENDER), ((J, None, p, p, p), NO_DEVICE, RENDER)]),
        "rm_render_attach_diagnostics": ((p,), HOST, [((odd,), NO_DEVICE, HOST)]),
        "rm_assemble_frame_device": ((p, 64, 0, 16, 4, 4, ids, 1, 1, p, -1, None, None), HOST,
                                     [((None, 64, 0, 16, 4, 4, ids, 1, 1, p, -1, None, None), NO_DEVICE, HOST),
                                      ((p, 64, 0, 16, 4, 4, ids, 1, 0, p, -1, None, None), NO_DEVICE, HOST)]),
        "rm_shade": ((0, 4, 4) + five, HOST, [((0, -4, 4) + five, NO_DEVICE, HOST), ((0, 4, 4, None, p, p, p, p), NO_DEVICE, HOST)]),
        "rm_shade_device": ((0, 4, 4) + five + (None,), HOST,
                            [((0, 4, -4) + five + (None,), NO_DEVICE, HOST), ((0, 4, 4, p, p, p, p, None, None), NO_DEVICE, HOST)]),
        "rm_reduce_counters_enqueue": ((p, p, 16, p, None), HOST, [((p, p, 16, None, None), INVALID, KEPT), ((p, p, -1, p, None), NO_DEVICE, HOST),
                                                                    ((None, p, 16, p, None), NO_DEVICE, HOST)]),
        "rm_reduce_counters_device": ((p, p, 16, D, None), HOST, [((p, p, 16, None, None), INVALID, KEPT), ((p, p, -1, D, None), NO_DEVICE, HOST)]),
        "rm_reduce_counters": ((p, p, 16, D), HOST, [((p, p, 16, None), INVALID, KEPT), ((p, None, 16, D), NO_DEVICE, HOST), ((p, p, -1, D), NO_DEVICE, HOST)]),
        "rm_scene_distance": ((p, 4, p, p), HOST, [((p, -1, p, p), NO_DEVICE, HOST), ((None, 4, p, p), NO_DEVICE, HOST)]),
        "rm_ray_march": rays(False, False),
        "rm_ray_march_device": rays(True, False),
        "rm_ray_pick": rays(False, True),
        "rm_ray_pick_device": rays(True, True),
        "rm_selftest_hypot": ((p, 4, p), HOST, [((p, -1, p), NO_DEVICE, HOST), ((None, 4, p), NO_DEVICE, HOST)]),
        "rm_selftest_jsmath": ((0, p, p, 4, p), HOST, [((9, p, p, 4, p), NO_DEVICE, HOST), ((0, None, p, 4, p), NO_DEVICE, HOST)]),
        "rm_selftest_fastdiv": ((1, 4, U), HOST, [((1, 4, None), INVALID, KEPT), ((1, -4, U), NO_DEVICE, HOST)]),
        "rm_selftest_recip": ((0, p), HOST, [((0, None), INVALID, KEPT), ((2, p), NO_DEVICE, HOST)]),
        "rm_debug_read_stamps": ((p,), HOST, [((None,), INVALID, KEPT)]),
        "rm_debug_read_wave_times": ((p,), HOST, [((None,), INVALID, KEPT)]),
        "rm_debug_read_batch_log": ((p,), HOST, [((None,), INVALID, KEPT)]),
        "rm_debug_read_counts": ((p,), HOST, [((None,), INVALID, KEPT)]),
        "rm_debug_read_lpt_costs": ((p, 16), HOST, [((None, 16), INVALID, KEPT), ((p, -1), NO_DEVICE, HOST)]),
    }
    assert len(table) == 25 and set(table) <= set(N.SIGNATURES)
    for name, (good, text, bad) in table.items():
        fn = getattr(L, name)
        assert fn(None, *good) == INVALID, name  # a null context: no context to leave a text in
        for args, code, want in [(good, NO_DEVICE, text)] + bad:
            assert L.rm_set_option(ctx._h, b"no_such_option", 1) == INVALID
            assert fn(ctx._h, *args) == code, (name, args)
            assert L.rm_last_error(ctx._h).decode() == want, (name, args)
    ctx.close()
