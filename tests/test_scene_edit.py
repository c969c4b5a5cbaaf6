"""rm_scene_edit_spheres on a host-only context (no GPU): an edit leaves what rm_scene_from_spheres(edited list) leaves -- every
scene table and rm_scene_get_info --, the error codes, all or nothing; the Python and JS mirrors; and the register budget of
the device builder's kernels (csrc/rm_scene_build.hip).  tests/test_scene_edit_gpu.py has the device side."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_edit_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cpu_raymarcher_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NODE = shutil.which("node")
ACCELS = [M.BVH, M.OCTREE, M.NONE]

START = M.random_spheres(40, seed=11)
NEW = [((0.31, -0.72, 0.05), 0.22), ((-1.1, 0.4, 0.9), 0.08), ((0.0, 0.0, 0.0), 0.4)]
EDITS = {
    "set": [("set", 17, *NEW[0])],
    "insert_front": [("insert", 0, *NEW[0])],
    "insert_middle": [("insert", 20, *NEW[1])],
    "insert_end": [("insert", 40, *NEW[2])],
    "remove": [("remove", 5)],
    # later indices depend on earlier edits: 39 is the last entry only after the first removal, 40 the end only after the insert
    "mixed": [("remove", 0), ("set", 38, *NEW[0]), ("insert", 39, *NEW[1]), ("insert", 40, *NEW[2]), ("remove", 40), ("set", 0, *NEW[2])],
}


@pytest.fixture(scope="module")
def pair(rm):
    """Two host-only contexts: the one that is edited and the one that uploads the edited list."""
    a, b = rm.Context(None), rm.Context(None)
    yield a, b
    a.close()
    b.close()


def check_edit(pair, accel, start, edits):
    edited, fresh = pair
    edited.scene_from_spheres(start[0], start[1], accel)
    edited.edit_spheres(edits)
    want = M.apply_edits(start[0], start[1], edits)
    fresh.scene_from_spheres(want[0], want[1], accel)
    M.assert_same(M.snapshot(edited, False), M.snapshot(fresh, False), "accel %d" % accel)
    return want


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("case", sorted(EDITS))
def test_an_edit_leaves_what_an_upload_of_the_edited_list_leaves(pair, accel, case):
    check_edit(pair, accel, START, EDITS[case])


@pytest.mark.parametrize("accel", ACCELS)
def test_removing_every_sphere_and_inserting_them_back(pair, accel):
    start = M.random_spheres(3, seed=5)
    check_edit(pair, accel, start, [("remove", 2), ("remove", 0), ("remove", 0)])
    assert pair[0].scene_info()["n_prims"] == 0
    back = [("insert", 0, start[0][1], start[1][1]), ("insert", 0, start[0][0], start[1][0]), ("insert", 2, start[0][2], start[1][2])]
    pair[0].edit_spheres(back)  # on the empty scene the first edit left
    pair[1].scene_from_spheres(start[0], start[1], accel)
    M.assert_same(M.snapshot(pair[0], False), M.snapshot(pair[1], False))


@pytest.mark.parametrize("accel", ACCELS)
def test_an_edited_preset_is_the_uploaded_scene(rm, pair, accel):
    edited, fresh = pair
    edited.scene_from_preset(3, accel)
    assert edited.scene_info()["preset_index"] == 3
    edit = [("set", 62, (0.07, -0.03, 0.11), 0.15)]
    edited.edit_spheres(edit)
    want = M.apply_edits(*M.dense_grid(), edit)
    fresh.scene_from_spheres(want[0], want[1], accel)
    assert edited.scene_info()["preset_index"] == rm.context.N.RM_SCENE_UPLOADED
    M.assert_same(M.snapshot(edited, False), M.snapshot(fresh, False))
    # a second edit starts from the edited list, not from the preset
    edited.edit_spheres([("remove", 0)])
    want = M.apply_edits(want[0], want[1], [("remove", 0)])
    fresh.scene_from_spheres(want[0], want[1], accel)
    M.assert_same(M.snapshot(edited, False), M.snapshot(fresh, False))


def test_a_rebuild_of_the_uploaded_scene_takes_the_edited_list(rm, pair):
    """The remembered upload is the edited list: rm_set_option("length") rebuilds the active scene from it, as a job that names
    another acceleration structure does (tests/test_scene_edit_gpu.py renders one)."""
    edited, fresh = pair
    want = check_edit(pair, M.BVH, START, EDITS["mixed"])
    for ctx in pair:
        ctx.set_option("length", 1)  # rebuilds the active uploaded scene from what the context remembers
    try:
        M.assert_same(M.snapshot(edited, False), M.snapshot(fresh, False))
        assert edited.scene_info()["n_prims"] == len(want[1])
    finally:
        for ctx in pair:
            ctx.set_option("length", 0)


def raw_edit(op=0, index=0, center=(0.0, 0.0, 0.0), radius=0.1, reserved=0):
    N = sys.modules["cpu_raymarcher_amd._native"]
    e = (N.rm_sphere_edit * 1)()
    e[0].op, e[0].index, e[0].reserved, e[0].radius = op, index, reserved, radius
    e[0].center[:] = center
    return e


def test_error_codes(rm):
    N = rm.context.N
    L = N.lib()
    ctx = rm.Context(None)
    h = ctx._h
    one = raw_edit()
    assert L.rm_scene_edit_spheres(None, one, 1) == N.RM_E_INVALID
    assert L.rm_scene_edit_spheres(h, one, 1) == N.RM_E_NO_SCENE  # before any scene
    assert L.rm_scene_edit_spheres(h, raw_edit(op=7), 1) == N.RM_E_INVALID  # argument errors come ahead of it
    ctx.scene_from_spheres(START[0], START[1], M.BVH)
    before = M.snapshot(ctx, False)
    inf, nan = float("inf"), float("nan")
    bad = [(None, 1), (one, -1), (raw_edit(op=3), 1), (raw_edit(op=-1), 1), (raw_edit(reserved=1), 1),
           (raw_edit(op=0, index=40), 1), (raw_edit(op=0, index=-1), 1), (raw_edit(op=1, index=41), 1), (raw_edit(op=2, index=40), 1),
           (raw_edit(op=0, center=(nan, 0, 0)), 1), (raw_edit(op=1, center=(0, inf, 0)), 1), (raw_edit(op=0, radius=nan), 1),
           (raw_edit(op=1, radius=inf), 1)]
    for edits, n in bad:
        assert L.rm_scene_edit_spheres(h, edits, n) == N.RM_E_INVALID, (n, edits and (edits[0].op, edits[0].index))
        assert L.rm_last_error(h)
    assert L.rm_scene_edit_spheres(h, raw_edit(op=2, center=(nan, nan, nan), radius=nan), 1) == N.RM_OK  # REMOVE ignores them
    ctx.scene_from_spheres(START[0], START[1], M.BVH)
    assert L.rm_scene_edit_spheres(h, None, 0) == N.RM_OK and L.rm_scene_edit_spheres(h, one, 0) == N.RM_OK  # nothing to do
    M.assert_same(M.snapshot(ctx, False), before)
    # primitive lists, forests and presets 5 .. 18 keep no candidate tables
    ident = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    ctx.scene_from_prims([(1, ident, (0.5, 0.5, 0.5))], M.BVH)
    assert L.rm_scene_edit_spheres(h, one, 1) == N.RM_E_UNSUPPORTED
    ctx.scene_from_nodes([(0, -1, -1, ident, (0.5,))], [0], M.BVH)
    assert L.rm_scene_edit_spheres(h, one, 1) == N.RM_E_UNSUPPORTED
    for preset in (5, 6, 18):
        ctx.scene_from_preset(preset, M.BVH)
        assert L.rm_scene_edit_spheres(h, one, 1) == N.RM_E_UNSUPPORTED
    ctx.scene_from_preset(0, M.BVH)  # a sphere preset while a forest is the remembered upload: the preset is edited
    assert L.rm_scene_edit_spheres(h, one, 1) == N.RM_OK and ctx.scene_info()["n_prims"] == 1
    with pytest.raises(N.RmError):
        ctx.scene_table("no_such_table", from_device=False)
    with pytest.raises(N.RmError):
        ctx.scene_table("spheres", from_device=True)  # a host-only context has no device copy
    ctx.close()


@pytest.mark.parametrize("accel", ACCELS)
def test_all_or_nothing(rm, pair, accel):
    N = rm.context.N
    ctx = pair[0]
    ctx.scene_from_spheres(START[0], START[1], accel)
    before = M.snapshot(ctx, False)
    batch = EDITS["mixed"] + [("remove", 40)]  # 40 spheres remain: the last edit is out of range at its turn
    with pytest.raises(N.RmError) as err:
        ctx.edit_spheres(batch)
    assert err.value.code == N.RM_E_INVALID
    M.assert_same(M.snapshot(ctx, False), before)
    # ... and the remembered upload is the old list too
    ctx.set_option("length", 1)
    ctx.set_option("length", 0)
    M.assert_same(M.snapshot(ctx, False), before)


def test_option_device_build_is_a_switch(rm):
    ctx = rm.Context(None)
    assert ctx.get_option("device_build") == 1
    ctx.set_option("device_build", 0)
    assert ctx.get_option("device_build") == 0
    ctx.set_option("device_build", 5)
    assert ctx.get_option("device_build") == 1
    ctx.close()


def test_python_mirror(rm):
    ctx = rm.Context(None)
    scene = rm.Scene("BVH", ctx=ctx)
    scene.loadPreset(3)
    scene.setSphere(62, (0.07, -0.03, 0.11), 0.15)
    scene.insertSphere(0, (2.0, 0.0, 0.0), 0.3)
    scene.removeSphere(125)
    scene.editSpheres([("set", 1, (-2.0, 0.5, 0.0), 0.25), ("remove", 2)])
    assert scene.preset_for_job == rm.context.N.RM_SCENE_UPLOADED and scene.info()["n_prims"] == 124
    want = M.apply_edits(*M.dense_grid(), [("set", 62, (0.07, -0.03, 0.11), 0.15), ("insert", 0, (2.0, 0.0, 0.0), 0.3), ("remove", 125),
                                           ("set", 1, (-2.0, 0.5, 0.0), 0.25), ("remove", 2)])
    fresh = rm.Context(None)
    fresh.scene_from_spheres(want[0], want[1], M.BVH)
    M.assert_same(M.snapshot(ctx, False), M.snapshot(fresh, False))
    fresh.close()
    ctx.close()


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
def test_addon_edits_a_scene(rm):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "native")])
    addon = os.path.join(ROOT, "native", "build", "rm_addon.node")
    js = ("const a=require(%r);a.create(-1);const out=[];"
          "out.push(a.editSpheres(3,'BVH',new Int32Array([0,62,1,0,2,5]),new Float64Array([0.07,-0.03,0.11,0.15, 2,0,0,0.3, 0,0,0,0])));"
          "out.push(a.sceneInfo());"
          "out.push(a.editSpheres(-2147483648,'BVH',new Int32Array([2,0]),new Float64Array(4)));out.push(a.sceneInfo());"
          "out.push(a.editSpheres(-2147483648,'BVH',new Int32Array([0,500]),new Float64Array(4)));out.push(a.sceneInfo().nPrims);"
          "out.push(a.editSpheres(5,'BVH',new Int32Array([2,0]),new Float64Array(4)));"
          "out.push(Object.keys(a).includes('editSpheres'));console.log(JSON.stringify(out))" % addon)
    out = json.loads(subprocess.check_output([NODE, "-e", js]))
    uploaded = -2 ** 31
    assert out == [0, {"nPrims": 125, "presetIndex": uploaded, "accel": M.BVH}, 0, {"nPrims": 124, "presetIndex": uploaded, "accel": M.BVH},
                   -1, 124, -2, False]


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="hipcc / c++filt not present")
def test_device_builder_kernels_use_no_spill_and_no_scratch():
    """The sibling of tests/test_build_invariants.py for csrc/rm_scene_build.hip, with the Makefile's flags."""
    with tempfile.TemporaryDirectory() as tmp:
        remarks = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-S",
                                  "--cuda-device-only", "-mllvm", "-amdgpu-inline-max-bb=100000", "-Rpass-analysis=kernel-resource-usage",
                                  "-o", os.path.join(tmp, "listing.s"), os.path.join(CSRC, "rm_scene_build.hip")],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, check=True).stdout.decode()
    rows, cur = [], None
    for line in remarks.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        for key in ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur is not None and key not in cur:
                cur[key] = int(m.group(1))
    names = subprocess.check_output(["c++filt"] + [r["name"] for r in rows]).decode()
    for kernel in ("cand_count_kernel", "cand_fill_kernel<unsigned short>", "cand_fill_kernel<unsigned char>", "empty_dist_kernel",
                   "hypot64_kernel"):
        assert kernel in names, (kernel, names)
    for r in rows:
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read() and "rm_scene_build.hip" in open(os.path.join(CSRC, "Makefile")).read()
