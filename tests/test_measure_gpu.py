"""Measures on the GPU (rm_measure_field_device, rm_measure_tiles_device, Context.measure, MeshSession.measure;
include/rm_raymarch.h, "measures").  Everything measured is an integer: the dense record must equal tests/measure_model.py's of
the same values copied back, the sparse record the dense one of the exact field, field by field.  The only tolerance is the
shell bound of the sphere's volume, derived in that test."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, OCTREE, BVH = 0, 1, 2


def spheres40():
    rng = np.random.default_rng(40)
    return rng.uniform(-1.5, 1.5, (40, 3)).astype(np.float32), rng.uniform(0.05, 0.25, 40)


def load(ctx, scene, accel):
    if scene == "sphere":
        ctx.scene_from_preset(0, accel)  # one sphere of radius 1.5 about the origin
    else:
        ctx.scene_from_spheres(*spheres40(), accel)


def box(lo, hi, shape):
    """An axis-aligned lattice of `shape` points over [lo, hi]^3 (a count of 1: the plane at lo)."""
    step = [(hi - lo) / (n - 1) if n > 1 else 1.0 for n in shape]
    return ((lo, lo, lo), (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), shape)


# the shapes of tests/test_measure.py -- one block with its last point, a second block of one cell, two whole blocks, three, an
# anisotropic one, 4 x 4 x 4 blocks -- over [-2, 2]^3, a skewed left-handed lattice, and a slice
SKEWED = ((-2.0, -2.05, 2.0), (0.125, 0.004, -0.003), (-0.005, 0.125, 0.006), (0.004, -0.003, -0.125), (33, 33, 33))
VOLUMES = [box(-2.0, 2.0, s) for s in ((9, 9, 9), (10, 10, 10), (17, 17, 17), (18, 18, 18), (25, 13, 20), (33, 33, 33))] + [SKEWED]
SLICE = ((-2.0, -2.0, 0.1), (4.0 / 36, 0, 0), (0, 4.0 / 28, 0), (0, 0, 1.0), (37, 29, 1))
SCENES = [("sphere", BVH), ("sphere", OCTREE), ("spheres40", BVH), ("spheres40", OCTREE)]


@pytest.fixture(scope="module")
def mctx(rm):
    """A context of its own.  Interpreter only, like the field tests': every launch here is ahead-of-time."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    yield c
    c.close()


def as_dict(m):
    return dict(m._asdict())


def assert_world(rm, geom, m):
    """`.world` is rm_measure_world of the record on the lattice, which tests/test_measure.py holds to the model bit for bit."""
    want = M.world(geom[:4], as_dict(m))
    assert m.world.volume == want["volume"] and m.world.projected_area == want["projected_area"] and m.world.second == want["second"]
    assert m.inertia().shape == (3, 3) and np.allclose(m.inertia(), m.inertia().T)


@pytest.mark.parametrize("scene,accel", SCENES)
def test_measure_field_equals_the_model_on_the_values_copied_back(rm, mctx, scene, accel):
    load(mctx, scene, accel)
    for geom in VOLUMES + [SLICE]:
        nu, nv, nw = geom[4]
        for dist32 in (False, True):
            vol, _ = mctx.field(*geom, count=False, dist32=dist32, device=True)
            got = mctx.measure_field(vol, *geom, iso=0.0)
            want = M.measure_dense(vol.cpu().numpy(), nu, nv, nw, 0.0)
            assert as_dict(got) == want, (geom[4], dist32, got, want)
            assert (got.n_inside > 0 or nu < 25) and got.n_blocks == 0 and got.n_kept == 0
            assert mctx.last_kernel() == "measure_field_kernel<%s>" % ("float" if dist32 else "double")
            assert_world(rm, geom, got)
    assert got.crossings[2] == 0 and got.lo[2] == got.hi[2] == 0  # the slice came last
    # a numpy array is uploaded; NaN and infinities are counted and lie outside; equality with iso is outside
    rng = np.random.default_rng(7)
    v = rng.standard_normal(21 * 10 * 67)
    v[::5] = 0.25
    v[3], v[11], v[20] = float("nan"), float("inf"), float("-inf")
    for values in (v, v.astype(np.float32)):
        got = mctx.measure_field(values, *box(-1.0, 1.0, (67, 10, 21)), iso=0.25)
        assert as_dict(got) == M.measure_dense(values, 67, 10, 21, 0.25) and got.n_nonfinite == 3
    # a lattice without points: zero sums, the empty box
    got = mctx.measure_field(np.zeros(0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (5, 0, 3))
    assert as_dict(got) == M.measure_dense(np.zeros(0), 5, 0, 3, 0.0) and got.lo == (M.INT32_MAX,) * 3 and got.hi == (-1, -1, -1)
    assert mctx.last_kernel() == "measure_final_kernel"


@pytest.mark.parametrize("scene,accel", SCENES)
def test_the_sparse_measure_equals_the_dense_one_of_the_exact_field(rm, mctx, scene, accel):
    load(mctx, scene, accel)
    # [-8, 8]^3 at 33^3: blocks 4 wide, so the far ones are dropped as outside
    wide = box(-8.0, 8.0, (33, 33, 33))
    for geom, iso in [(g, 0.0) for g in VOLUMES] + [(VOLUMES[2], 0.1), (VOLUMES[5], 0.1), (wide, 0.0), (wide, 0.1)]:
        sparse = mctx.measure(*geom, iso=iso, sparse=True)
        assert mctx.last_kernel() == "measure_tiles_kernel"
        dense = mctx.measure(*geom, iso=iso, sparse=False, exact=True)
        assert M.same_measure(as_dict(sparse), as_dict(dense)), (geom[4], iso, sparse, dense)
        assert dense.n_inside > 0 or geom is wide or geom[4][0] < 25
        # (9^3 is one block and the small lattices over [-2, 2]^3 keep every block: n_kept < n_blocks holds, and is asserted,
        # on the wide lattice below and in the large-sphere test, where blocks are dropped as outside and as inside)
        assert sparse.n_blocks == int(np.prod([(n + 6) // 8 for n in geom[4]])) and 0 < sparse.n_kept <= sparse.n_blocks
        assert_world(rm, geom, sparse)
        if geom is wide:
            assert sparse.n_kept < sparse.n_blocks and sparse.n_blocks_inside == 0
    assert mctx.get_option("exact") == 0  # the option is as it was


def test_blocks_deep_inside_a_large_sphere_take_the_closed_forms(rm, mctx):
    """33^3 over [-1, 1]^3 inside the sphere of radius 1.5: blocks 0.5 wide, bound 0.75; the eight central blocks have their
    centres 0.43 from the origin, 1.07 deep: dropped as inside."""
    geom = box(-1.0, 1.0, (33, 33, 33))
    for accel in (BVH, OCTREE, NONE):
        load(mctx, "sphere", accel)
        for iso in (0.0, 0.1):
            sparse, dense = mctx.measure(*geom, iso=iso), mctx.measure(*geom, iso=iso, sparse=False)
            assert M.same_measure(as_dict(sparse), as_dict(dense)), (accel, iso, sparse, dense)
            assert sparse.n_blocks_inside >= 8 and sparse.n_kept < sparse.n_blocks == 64
            assert sparse.n_kept + sparse.n_blocks_inside == 64  # no block of this lattice is dropped as outside
    # Scene.measure and Context.measure_box reach the same entries
    sc = rm.Scene("BVH", ctx=mctx)
    sc.loadPreset(0)
    assert sc.measure(*geom) == mctx.measure(*geom)
    m = sc.measure(cells=(40, 40, 40))
    assert m == mctx.measure_box((40, 40, 40)) and m.n_points == 41 ** 3 and 0 < m.n_inside < m.n_points


def test_a_centred_sphere_is_symmetric_and_has_its_volume(rm, mctx):
    """One sphere of radius 1.5 about the origin on the lattice origin -2, step 0.0625, 65^3: the points are exactly symmetric
    about index 32, and squares do not see a sign, so the inside set is too.  Hence 2 sum1 = 64 N, the mixed second sums are
    32^2 N, lo + hi = 64.  Volume: a point and its cell-sized box can disagree about the sphere only when the box meets the
    surface, so every misclassified cell lies within half a cell diagonal, sqrt(3) h / 2, of it; that shell, sqrt(3) h thick,
    has the volume 4 pi r^2 * sqrt(3) h to first order, which is 3 sqrt(3) h / r times the ball's: the bound.  (Measured:
    14.098389 against 14.137167, 0.27 % off; the bound allows 21.7 %.)"""
    load(mctx, "sphere", BVH)
    h, r = 0.0625, 1.5
    geom = box(-2.0, 2.0, (65, 65, 65))
    sparse, dense = mctx.measure(*geom), mctx.measure(*geom, sparse=False)
    assert M.same_measure(as_dict(sparse), as_dict(dense))
    for m in (sparse, dense):
        n = m.n_inside
        assert n > 0 and all(2 * s == 64 * n for s in m.sum1) and all(s == 32 * 32 * n for s in m.sum2[3:])
        assert all(a + b == 64 for a, b in zip(m.lo, m.hi)) and m.crossings[0] == m.crossings[1] == m.crossings[2] > 0
        ball = 4.0 / 3.0 * math.pi * r ** 3
        print("volume %.6f, ball %.6f, bound %.6f" % (m.world.volume, ball, 3 * math.sqrt(3) * h / r * ball))
        assert m.world.cell_volume == h ** 3 and abs(m.world.volume - ball) <= 3 * math.sqrt(3) * h / r * ball
        assert m.world.centroid == (0.0, 0.0, 0.0)
        # the projected area of a convex body along an axis is twice its shadow; the estimate is the sphere's area within the shell bound's order
        assert all(abs(p - 2 * math.pi * r * r) <= 3 * math.sqrt(3) * h / r * 2 * math.pi * r * r for p in m.world.projected_area)
        inertia = m.inertia()
        assert np.allclose(inertia, np.diag(np.diag(inertia)), atol=1e-9) and inertia[0, 0] > 0


def test_a_session_measures_its_current_tiles(rm, mctx):
    mctx.scene_from_spheres(*spheres40(), BVH)
    geom = box(-2.0, 2.0, (33, 33, 33))
    s = mctx.mesh_session(*geom)
    before = s.measure()
    assert before == mctx.measure(*geom)
    centers, radii = spheres40()
    s.edit_spheres([("set", 7, centers[7].astype(np.float64) + (0.3, -0.2, 0.25), 0.4)])
    after = s.measure()
    assert s.stats["n_reused"] > 0 and s.stats["n_evaluated"] > 0  # copied tiles are among those measured
    assert mctx.last_kernel() == "measure_tiles_kernel"
    scratch = mctx.measure(*geom)
    assert after == scratch and as_dict(after) == as_dict(scratch)
    assert after != before and after.n_inside != before.n_inside
    assert M.same_measure(as_dict(after), as_dict(mctx.measure(*geom, sparse=False)))


def test_two_calls_on_a_side_stream_leave_nothing_behind(rm, mctx):
    import torch
    mctx.scene_from_spheres(*spheres40(), OCTREE)
    geom = VOLUMES[4]
    vol, _ = mctx.field(*geom, count=False, device=True, exact=True)
    want = M.measure_dense(vol.cpu().numpy(), *geom[4], 0.05)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        first, second = mctx.measure_field(vol, *geom, iso=0.05), mctx.measure_field(vol, *geom, iso=0.05)
        sparse = [mctx.measure(*geom, iso=0.05) for _ in range(2)]
    side.synchronize()
    assert as_dict(first) == as_dict(second) == want
    assert sparse[0] == sparse[1] and M.same_measure(as_dict(sparse[0]), want)


# ------------------------------------------------------------------------------------------------- the host entry

NO_SCENE = -5


def host_measure(rm, ctx, geom, iso=0.0, time=0.0, lipschitz=1.0):
    """rm_scene_measure through ctypes, the record and the info filled with 0xA5 bytes first -> (Measure, rm_measure, rm_sparse_info)."""
    N = rm._native
    lat = rm.make_lattice(*geom, time)
    out, info = N.rm_measure(), N.rm_sparse_info()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    N.check(ctx._h, N.lib().rm_scene_measure(ctx._h, C.byref(lat), float(iso), float(lipschitz), C.byref(out), C.byref(info)))
    return rm.context.measure_from_record(lat, out), out, info


def assert_host_equals_python(rm, ctx, geom, iso, time=0.0, reference=None):
    """The host entry's record is Context.measure(sparse=True)'s field by field, the block fields included; every field is
    written; sparse_info says what the record says."""
    got, raw, info = host_measure(rm, ctx, geom, iso, time)
    want = (reference or ctx).measure(*geom, iso=iso, time=time)
    assert as_dict(got) == as_dict(want), (geom[4], iso, got, want)
    assert raw.reserved == 0 and raw.n_points == int(np.prod(geom[4]))
    assert (info.n_blocks, info.n_kept, list(info.reserved)) == (got.n_blocks, got.n_kept, [0, 0])
    return got


@pytest.mark.parametrize("scene,accel", SCENES)
def test_the_host_entry_equals_the_three_device_steps(rm, mctx, scene, accel):
    """rm_scene_measure on the scenes and shapes above.  Option exact is 0 throughout: under the octree the scene's own field is
    the marchers' bound, so equality with Context.measure -- and with the dense measure of the exact field -- shows that the
    entry's tiles hold the exact field whatever the option says."""
    load(mctx, scene, accel)
    assert mctx.get_option("exact") == 0
    wide = box(-8.0, 8.0, (33, 33, 33))
    for geom, iso in [(g, 0.0) for g in VOLUMES] + [(VOLUMES[5], 0.1), (wide, 0.0), (wide, 0.1)]:
        got = assert_host_equals_python(rm, mctx, geom, iso)
        assert mctx.last_kernel() == "measure_tiles_kernel"
        assert M.same_measure(as_dict(got), as_dict(mctx.measure(*geom, iso=iso, sparse=False, exact=True)))
    assert mctx.get_option("exact") == 0


def test_the_host_entry_on_a_fresh_context_grows_the_scratch_between_its_steps(rm, mctx):
    """The first call of a context whose scratch is empty: the coarse pass reserves some kilobytes, the tiles need megabytes, so
    the slot map, the list and the distances cross the host while the scratch grows.  Then a second call that need not grow.
    Blocks dropped as inside (the sphere over [-1, 1]^3) and as outside (the 40 spheres over [-8, 8]^3) are among them."""
    cases = [("sphere", OCTREE, box(-1.0, 1.0, (33, 33, 33)), 0.1), ("spheres40", BVH, box(-8.0, 8.0, (33, 33, 33)), 0.0),
             ("spheres40", OCTREE, SKEWED, 0.0)]
    for scene, accel, geom, iso in cases:
        load(mctx, scene, accel)
        with rm.Context(0) as fresh:
            fresh.set_option("specialise", 0)
            load(fresh, scene, accel)
            for _ in range(2):
                got = assert_host_equals_python(rm, fresh, geom, iso, reference=mctx)
            assert got.n_kept > 0 and fresh.get_option("exact") == 0


def test_the_host_entry_takes_the_lattices_time_and_leaves_the_scenes(rm, mctx):
    """Preset 12 moves a sphere along x with time.  The record follows lattice->time; rm_scene_set_time's value, option exact
    and an armed diagnostics accumulator are as they were; without a scene the entry says so, last."""
    import torch
    N = rm._native
    mctx.scene_from_preset(12, BVH)
    mctx.scene_set_time(0.9)
    geom = box(-4.0, 4.0, (33, 33, 33))
    pts = np.random.default_rng(3).uniform(-3.0, 3.0, (32, 3)).astype(np.float32)
    at_09 = mctx.scene_distance(pts)[0]
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    mctx._attach_diag(acc)
    early = assert_host_equals_python(rm, mctx, geom, 0.0, time=0.0)
    late = assert_host_equals_python(rm, mctx, geom, 0.0, time=200.0)
    assert early.n_inside > 0 and late.n_inside > 0 and early.sum1[0] != late.sum1[0]
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "the measure fired the diagnostics"
    assert mctx.scene_distance(pts)[0].tobytes() == at_09.tobytes() and mctx.get_option("exact") == 0
    # no scene: RM_E_NO_SCENE, behind the argument checks
    with rm.Context(0) as empty:
        lat = rm.make_lattice(*geom)
        out = N.rm_measure()
        L = N.lib()
        assert L.rm_scene_measure(empty._h, C.byref(lat), 0.0, 1.0, C.byref(out), None) == NO_SCENE
        assert L.rm_scene_measure(empty._h, C.byref(lat), 0.0, 0.0, C.byref(out), None) == -1
        assert L.rm_scene_measure(empty._h, C.byref(lat), 0.0, 1.0, None, None) == -1
