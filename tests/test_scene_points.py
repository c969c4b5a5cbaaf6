"""Point queries (rm_scene_points / rm_scene_points_device; Context.points, project, the meshers' attributes, save_obj).
CPU tests: the numpy model of the rule (point_model.py) against the oracle, the ABI contract on a host-only context, the
build invariants of every point_kernel instantiation, the OBJ writer.  GPU tests: with K = 0 the query is rm_scene_distance;
at the hit points of a ray query its normal, object and count are the ray queries'; projections equal the model byte for
byte; objects agree with single-object scenes; the device entry equals the host entry; a host batch crosses the chunk; the
meshers' attributes are the model's.  There are no tolerances: every comparison is of bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import point_model as M  # noqa: E402

ACCELS = ("None", "Octree", "BVH")
ACCEL_ENUM = {"None": 0, "Octree": 1, "BVH": 2}
# one scene of each kind point_kernel is instantiated for: sphere list, primitive list, expression forest, forest with the Mandelbulb
KINDS = {"spheres": 3, "prims": 9, "forest": 10, "mandelbulb": 13}
FILL = 0xA5


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def query(rm, snap=0, tol=1e-4, iso=0.0, time=0.0, flags=0, reserved=(0, 0)):
    q = rm._native.rm_point_query()
    q.time, q.iso, q.snap_tol, q.snap_steps, q.flags = time, iso, tol, snap, flags
    q.reserved[0], q.reserved[1] = reserved
    return q


def near_surface(D, rng, n, lo, hi, within=0.5, iso=0.0):
    """n random float32 points of the box [lo, hi] whose distance is within `within` of iso."""
    got = []
    while sum(len(g) for g in got) < n:
        p = rng.uniform(lo, hi, (4 * n, 3)).astype(np.float32)
        d, _ = D(p)
        got.append(p[np.abs(d - iso) < within])
    return np.concatenate(got)[:n]


def assert_equals_model(got, want, what):
    """position, dist, normal, steps, count of a Points tuple against the model's PointResult, byte for byte."""
    assert same_bits(got.position, want.position), (what, "position", int((got.position != want.position).any(axis=1).sum()))
    assert same_bits(got.dist, want.dist), (what, "dist")
    assert same_bits(got.normal, want.normal), (what, "normal")
    assert np.array_equal(got.steps, want.steps), (what, "steps")
    assert np.array_equal(got.count.astype(np.uint64), want.count), (what, "count")


# ------------------------------------------------------------------------------------------- CPU: the model and the oracle

def test_the_model_drops_points_onto_a_sphere_in_one_step(oracle):
    """Sphere preset / None: the distance is exact and its gradient the radial direction, so one step of -d along it lands on
    the surface (to binary32 rounding of the position)."""
    D = M.oracle_distance(oracle.OracleScene(preset=0, accel="None"))
    p = near_surface(D, np.random.default_rng(1), 100, -2.5, 2.5)
    r = M.points_model(D, p, snap=8, tol=1e-4)
    assert (r.steps == 1).all(), r.steps
    assert (np.abs(r.dist) <= 1e-4).all(), np.abs(r.dist).max()
    assert same_bits(r.dist, D(r.position)[0]) and (np.linalg.norm(r.normal.astype(np.float64), axis=1) > 0.999).all()
    assert (r.count == 1 + 4 + 3).all()  # D(p0); G there; D at the new point and, for the normal, G there


def _dense_grid_points(oracle, accel, n=120):
    """120 random points of [-2.5, 2.5]^3 within 0.5 of the surface by the scene's own getDistance."""
    D = M.oracle_distance(oracle.OracleScene(preset=3, accel=accel))
    return D, near_surface(D, np.random.default_rng(2), n, -2.5, 2.5)


def test_the_model_stops_at_once_in_an_empty_octree_leaf(oracle):
    """getDistance is taken as it is: an empty leaf answers a constant, so G is (0, 0, 0) and the projection ends with steps = 0."""
    D, p = _dense_grid_points(oracle, "Octree")
    d0, c0 = D(p)
    empty = c0 == 0  # inside the cube (outside it every primitive is evaluated), no primitive evaluated: an empty leaf
    assert 10 <= empty.sum() < len(p), int(empty.sum())
    r = M.points_model(D, p, snap=8, tol=1e-4)
    stuck = empty & (np.abs(d0) > 1e-4)
    assert stuck.sum() >= 10
    assert (r.steps[stuck] == 0).all() and not r.normal[stuck].any() and same_bits(r.position[stuck], p[stuck])
    assert same_bits(r.dist[stuck], d0[stuck])


@pytest.mark.parametrize("accel", ["None", "BVH"])
def test_the_model_leaves_no_point_unconverged_on_the_dense_grid(oracle, accel):
    D, p = _dense_grid_points(oracle, accel)
    r = M.points_model(D, p, snap=8, tol=1e-4)
    print("Dense Grid / %s: largest final |dist| %.3g, steps up to %d" % (accel, np.abs(r.dist).max(), r.steps.max()))
    assert (np.abs(r.dist) <= 1e-4).all(), (np.abs(r.dist).max(), int((np.abs(r.dist) > 1e-4).sum()))
    assert (r.steps >= 1).all() and (r.steps <= 8).all()


def test_the_model_without_steps_or_normal_is_one_evaluation(oracle):
    D = M.oracle_distance(oracle.OracleScene(preset=9, accel="BVH"))
    p = np.random.default_rng(3).uniform(-2, 2, (20, 3)).astype(np.float32)
    r = M.points_model(D, p, snap=0, normal=False)
    d, c = D(p)
    assert same_bits(r.position, p) and same_bits(r.dist, d) and np.array_equal(r.count, c) and not r.normal.any() and not r.steps.any()
    # K that runs out: one step taken where the start is off the surface, the distance taken at the new point
    r1 = M.points_model(D, p, snap=1, tol=0.0, normal=False)
    moved = (r1.position != p).any(axis=1)
    assert (r1.steps == moved).all() and moved.any() and same_bits(r1.dist, D(r1.position)[0])


# ------------------------------------------------------------------------------------------------- CPU: ABI contract

def test_the_library_exports_the_point_entries_and_the_query_has_its_size(rm):
    N = rm._native
    assert C.sizeof(N.rm_point_query) == 40 and N.RM_POINT_NORMAL == 1
    assert hasattr(N.lib(), "rm_scene_points") and hasattr(N.lib(), "rm_scene_points_device")


def test_bad_point_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)  # host-only, and no scene: every argument check comes first
    p = np.zeros((4, 3), np.float32)
    pos, dist, nrm = np.zeros((4, 3), np.float32), np.zeros(4, np.float64), np.zeros((4, 3), np.float32)
    obj, steps, cnt = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint32)
    outs = [pos, dist, nrm, obj, steps, cnt]

    def both(q, n, points, o):
        a = L.rm_scene_points(ctx._h, None if q is None else C.byref(q), n, vp(points), *[b if isinstance(b, C.c_void_p) else vp(b) for b in o])
        b = L.rm_scene_points_device(ctx._h, None if q is None else C.byref(q), n, vp(points), *[b if isinstance(b, C.c_void_p) else vp(b) for b in o], None)
        assert a == b, (a, b)
        return a

    ok = query(rm, snap=3, flags=N.RM_POINT_NORMAL)
    assert both(None, 4, p, outs) == N.RM_E_INVALID  # null query
    assert both(query(rm, reserved=(0, 1)), 4, p, outs) == N.RM_E_INVALID
    assert both(query(rm, reserved=(7, 0)), 4, p, outs) == N.RM_E_INVALID
    assert both(query(rm, flags=2), 4, p, outs) == N.RM_E_INVALID  # unknown flag bits
    assert both(query(rm, flags=-1), 4, p, outs) == N.RM_E_INVALID
    for k in (-1, 17, 2 ** 31 - 1):
        assert both(query(rm, snap=k), 4, p, outs) == N.RM_E_INVALID, k
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert both(query(rm, time=bad), 4, p, outs) == N.RM_E_INVALID
        assert both(query(rm, iso=bad), 4, p, outs) == N.RM_E_INVALID
        assert both(query(rm, tol=bad), 4, p, outs) == N.RM_E_INVALID
    assert both(query(rm, tol=-1e-9), 4, p, outs) == N.RM_E_INVALID
    assert both(ok, -1, p, outs) == N.RM_E_INVALID
    assert both(ok, 2 ** 31, p, outs) == N.RM_E_INVALID
    assert both(ok, 4, None, outs) == N.RM_E_INVALID  # null points
    assert both(ok, 4, p, [None] * 6) == N.RM_E_INVALID  # nothing asked for
    for k, align in enumerate((4, 8, 4, 4, 4, 4)):  # a misaligned output
        raw = np.zeros(64, np.uint8)
        o = [None] * 6
        o[k] = C.c_void_p(raw.ctypes.data + align // 2)
        assert both(ok, 4, p, o) == N.RM_E_INVALID, k
    for bad in (np.nan, np.inf):  # the host entry alone checks the points
        q = p.copy()
        q[3, 2] = bad
        assert L.rm_scene_points(ctx._h, C.byref(ok), 4, vp(q), *[vp(b) for b in outs]) == N.RM_E_INVALID
        assert L.rm_scene_points_device(ctx._h, C.byref(ok), 4, vp(q), *[vp(b) for b in outs], None) == N.RM_E_NO_DEVICE
    assert L.rm_scene_points(None, C.byref(ok), 4, vp(p), *[vp(b) for b in outs]) == N.RM_E_INVALID
    # well-formed arguments on a host-only context: no device (n == 0 asks for no buffer; as rm_scene_field, it still needs one)
    assert both(ok, 0, None, [None] * 6) == N.RM_E_NO_DEVICE
    assert both(ok, 4, p, outs) == N.RM_E_NO_DEVICE
    assert both(ok, 4, p, [None, dist, None, None, None, None]) == N.RM_E_NO_DEVICE
    assert both(query(rm, snap=16, tol=0.0), 4, p, outs) == N.RM_E_NO_DEVICE
    ctx.scene_from_preset(3, 2)
    assert both(ok, 4, p, outs) == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.points(p)
    assert e.value.code == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.points(p, device=True)
    assert e.value.code == N.RM_E_NO_DEVICE


# ------------------------------------------------------------------------------------------------- CPU: build invariants

@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_point_kernels_spill_nothing(extra):
    """Exactly twelve point_kernel<ACCEL, GEN>: no VGPR spill; no scratch for spheres and primitive lists (GEN 0 / 1); the
    expression-program interpreter's per-lane scratch (GEN 2 / 3) within the bound of the render and query kernels."""
    from test_build_invariants import HIPCC, assert_no_vgpr_spill, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void point_kernel<")}
    assert len(kernels) == 12, sorted(kernels)
    assert_no_vgpr_spill(kernels, 800)


# ------------------------------------------------------------------------------------------------------- CPU: save_obj

def read_obj(path):
    v, vn, faces, group = [], [], [], None
    for line in open(path):
        w = line.split()
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w[0] == "g":
            group = w[1]
        elif w[0] == "f":
            faces.append((group, [c for c in w[1:]]))
    return np.array(v, np.float64).astype(np.float32), np.array(vn, np.float64).astype(np.float32), faces


def test_save_obj_with_normals_and_objects(rm, tmp_path):
    rng = np.random.default_rng(5)
    v = rng.normal(size=(7, 3)).astype(np.float32)
    v[0] = [1 / 3, -0.0, 1e-20]
    quads = np.array([[0, 1, 2, 3], [4, 5, 6, 0], [2, 3, 4, 5], [6, 0, 1, 2], [5, 6, 1, 3]], np.uint32)
    # the default output is what the plain writer wrote
    rm.save_obj(tmp_path / "plain.obj", v, quads)
    want = "".join("v %r %r %r\n" % tuple(float(x) for x in row) for row in v) + "".join("f %d %d %d %d\n" % tuple(int(i) + 1 for i in row) for row in quads)
    assert open(tmp_path / "plain.obj").read() == want
    rm.save_obj(tmp_path / "tri.obj", v, quads[:, :3].astype(np.int32))
    assert open(tmp_path / "tri.obj").read().endswith("f 6 7 2\n")
    # normals and objects
    n = rng.normal(size=(7, 3)).astype(np.float32)
    obj = np.array([2, -1, 0, 2, 0, 2, -1], np.int32)
    rm.save_obj(tmp_path / "full.obj", v, quads, normals=n, objects=obj)
    rv, rn, faces = read_obj(tmp_path / "full.obj")
    assert same_bits(rv, v) and same_bits(rn, n)
    text = open(tmp_path / "full.obj").read()
    assert text.index("\nvn ") > text.rindex("\nv ") and text.index("\ng ") > text.rindex("\nvn ")
    first = obj[quads[:, 0]]  # 2, 0, 0, -1, 2
    order = np.argsort(first, kind="stable")
    assert [g for g, _ in faces] == ["background" if k < 0 else "object_%d" % k for k in first[order]]
    assert [g for g, _ in faces] == ["background", "object_0", "object_0", "object_2", "object_2"]
    assert [c for _, c in faces] == [["%d//%d" % (i + 1, i + 1) for i in quads[k]] for k in order]
    assert text.count("\ng ") == 3
    # normals alone: no groups, the faces in their order
    rm.save_obj(tmp_path / "n.obj", v, quads, normals=n)
    _, rn, faces = read_obj(tmp_path / "n.obj")
    assert same_bits(rn, n) and [g for g, _ in faces] == [None] * 5 and faces[1][1] == ["5//5", "6//6", "7//7", "1//1"]
    # objects alone: plain corners under groups
    rm.save_obj(tmp_path / "o.obj", v, quads, objects=obj)
    _, rn, faces = read_obj(tmp_path / "o.obj")
    assert len(rn) == 0 and faces[0] == ("background", ["7", "1", "2", "3"])
    with pytest.raises(ValueError):
        rm.save_obj(tmp_path / "bad.obj", v, quads, normals=n[:5])


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope="module")
def pctx(rm):
    """A context of its own.  Interpreter only: point_kernel is ahead-of-time, so is rm_scene_distance then."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    return c


@pytest.fixture(scope="module")
def octx(rm):
    """The single-object scenes of the object check (test_ray_pick.single_object_values)."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    return c


def load(rm, ctx, preset, accel):
    sc = rm.Scene(accel, ctx=ctx)
    sc.loadPreset(preset)
    return sc


_boxes = {}


def root_box(rm, preset):
    if preset not in _boxes:
        info = load(rm, rm.Context(None), preset, "BVH").info()
        _boxes[preset] = (np.array(info["root_min"], np.float64), np.array(info["root_max"], np.float64))
    return _boxes[preset]


def scene_points(rm, preset, n, seed, scale=1.5):
    """n random points of the scene's root box scaled by `scale` about its centre: inside objects, in empty octree leaves,
    in no BVH leaf box, outside the octree's cube."""
    mn, mx = root_box(rm, preset)
    c, h = (mn + mx) / 2, np.minimum((mx - mn) / 2, 2.2) * scale  # (a forest's root box is a loose bound: stay near the objects)
    return np.random.default_rng(seed).uniform(c - h, c + h, (n, 3)).astype(np.float32)


def check_objects(ctx, octx, res, time, what):
    """res.object against single-object scenes at res.position with D = res.dist (test_ray_pick's independent check)."""
    from test_ray_pick import expected_ids, single_object_values
    n_obj = ctx.scene_info()["n_prims"]
    v = single_object_values(ctx, octx, res.position, n_obj, time)
    want = expected_ids(res.dist, v, n_obj)
    # a single-object scene answers min(10, sdf) like any scene: where D is the start value 10 every object beyond 10 seems to
    # match.  There no Primitive.sdf equals D (it would have to be 10.0 exactly): the rule's answer is -1.
    want[res.dist == 10.0] = -1
    bad = res.object != want
    assert not bad.any(), (what, np.nonzero(bad)[0][:8], res.object[bad][:8], want[bad][:8])
    return set(res.object.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("kind,length", [("spheres", 0), ("spheres", 1), ("prims", 0), ("forest", 0), ("mandelbulb", 0)])
def test_without_steps_or_flags_it_is_scene_distance(rm, pctx, kind, length, accel):
    load(rm, pctx, KINDS[kind], accel)
    pctx.set_option("length", length)
    try:
        pts = scene_points(rm, KINDS[kind], 257, 10)
        want_d, want_c = pctx.scene_distance(pts)
        gen = {"spheres": 0, "prims": 1, "forest": 2, "mandelbulb": 3}[kind]
        for n in (1, 63, 64, 65, 255, 256, 257):
            r = pctx.points(pts[:n], normal=False, object=False)
            assert pctx.last_kernel() == "point_kernel<%d, %d>%s" % (ACCEL_ENUM[accel], gen, " [length=sqrt]" if length else ""), pctx.last_kernel()
            assert same_bits(r.dist, want_d[:n]) and np.array_equal(r.count, want_c[:n]), (kind, accel, n)
            assert same_bits(r.position, pts[:n]) and not r.steps.any() and r.normal is None and r.object is None
        assert want_c.max() > 0 and (kind in ("forest", "mandelbulb") or (want_d < 0).any())
    finally:
        pctx.set_option("length", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("preset", [3, 10])
def test_at_hit_points_normal_object_and_count_are_the_ray_queries(rm, pctx, preset, accel):
    from test_ray_pick import hit_points
    load(rm, pctx, preset, accel)
    org, dirs = rm.camera_rays(16, 16, 0.3, 0.7)
    o = np.ascontiguousarray(np.broadcast_to(org, dirs.shape))
    t, _, sdf1, nrm, obj = pctx.pick(o, dirs, normal=True)
    _, _, sdf0, _ = pctx.ray_march(o, dirs, normal=False)
    hit = t < 10
    assert hit.sum() >= 20, int(hit.sum())
    r = pctx.points(hit_points(o[hit], dirs[hit], t[hit]))
    assert same_bits(r.normal, nrm[hit]) and np.array_equal(r.object, obj[hit])
    assert np.array_equal(r.count, sdf1[hit] - sdf0[hit]) and not r.steps.any()


# (preset, accel, points, K, tol, iso, time, normal): the oracle's distances, about 200 points in all
ORACLE_CASES = [(3, "None", 24, 8, 1e-4, 0.0, 0.0, True), (3, "BVH", 24, 8, 1e-4, 0.0, 0.0, True), (3, "Octree", 24, 8, 1e-4, 0.0, 0.0, True),
                (9, "BVH", 24, 1, 1e-4, 0.0, 0.0, False), (9, "None", 24, 2, 1e-4, 0.0, 0.0, True), (9, "None", 16, 16, 0.0, 0.0, 0.0, True),
                (10, "BVH", 24, 4, 1e-4, 0.1, 0.0, True), (12, "Octree", 24, 4, 1e-4, 0.0, 0.7, True), (12, "None", 16, 4, 1e-4, 0.0, 0.7, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel,n,snap,tol,iso,time,normal", ORACLE_CASES)
def test_projections_equal_the_model_over_the_oracle(rm, oracle, pctx, octx, preset, accel, n, snap, tol, iso, time, normal):
    load(rm, pctx, preset, accel)
    pts = scene_points(rm, preset, n, 20 + preset)
    r = pctx.points(pts, normal=normal, snap=snap, tol=tol, iso=iso, time=time)
    want = M.points_model(M.oracle_distance(oracle.OracleScene(preset=preset, accel=accel), time), pts, snap, tol, iso, normal)
    if normal:
        assert_equals_model(r, want, (preset, accel))
    else:
        assert r.normal is None
        assert_equals_model(r._replace(normal=np.zeros((n, 3), np.float32)), want, (preset, accel))
    assert r.steps.max() > 0 and (snap > 2 or (r.steps == snap).any())  # some points move; a small K runs out
    check_objects(pctx, octx, r, time, (preset, accel))


# (preset, accel, K, tol, iso, time): Context.scene_distance's distances, 250 points each
CONTEXT_CASES = [(3, "None", 3, 1e-4, 0.0, 0.0), (3, "BVH", 8, 1e-4, 0.0, 0.0), (3, "Octree", 8, 1e-4, 0.0, 0.0), (9, "BVH", 1, 1e-4, 0.0, 0.0),
                 (9, "Octree", 2, 1e-4, 0.0, 0.0), (9, "None", 16, 0.0, 0.0, 0.0), (10, "None", 5, 1e-3, 0.1, 0.0), (12, "BVH", 4, 1e-4, 0.0, 0.7)]


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel,snap,tol,iso,time", CONTEXT_CASES)
def test_projections_equal_the_model_over_scene_distance(rm, pctx, octx, preset, accel, snap, tol, iso, time):
    load(rm, pctx, preset, accel)
    pts = scene_points(rm, preset, 250, 40 + preset)
    mn, mx = root_box(rm, preset)
    outside = ((pts < mn) | (pts > mx)).any(axis=1)
    assert preset == 12 or 20 <= outside.sum() <= 230  # outside the BVH's root box: in no leaf box (the animated preset's box is loose)
    pts[:6] = 10.5 * np.concatenate([np.eye(3), -np.eye(3)]) + pts[:6] / 4  # beyond each face of the octree's cube (20 a side)
    pctx.scene_set_time(time)
    d0, c0 = pctx.scene_distance(pts)
    grid = accel == "Octree" and preset == 3  # (the other presets' octrees are one leaf)
    if grid:
        assert (c0 == 0).sum() >= 10, "no point in an empty leaf"
        assert (c0 == pctx.scene_info()["n_prims"]).any(), "no point outside the cube"
    r = pctx.points(pts, snap=snap, tol=tol, iso=iso, time=time)
    want = M.points_model(M.context_distance(pctx, time), pts, snap, tol, iso, True)
    assert_equals_model(r, want, (preset, accel))
    assert (r.steps == snap).any() or snap > 2, "K never ran out"
    assert (r.steps > 0).any() and (r.steps < max(snap, 2)).any()
    if grid:  # an empty leaf: no gradient, no step
        stuck = (c0 == 0) & (np.abs(d0 - iso) > tol)
        assert stuck.any() and not r.steps[stuck].any() and not r.normal[stuck].any() and same_bits(r.position[stuck], pts[stuck])
    check_objects(pctx, octx, r, time, (preset, accel))
    # the snap alone, and the scene's own entry
    pos, dist, steps = pctx.project(pts, steps=snap, tol=tol, iso=iso, time=time)
    assert same_bits(pos, r.position) and same_bits(dist, r.dist) and np.array_equal(steps, r.steps)


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", ["mixed", "forest", 12])
def test_objects_agree_with_single_object_scenes(rm, oracle, pctx, octx, scene, accel):
    """A primitive list (40 mixed primitives), a forest of three objects (the roots of presets 18 and 11 side by side) and the
    animated preset -- at the points as given and after a projection."""
    time = 0.7 if scene == 12 else 0.0
    sc = rm.Scene(accel, ctx=pctx)
    if scene == 12:
        sc.loadPreset(scene)
        pts = scene_points(rm, scene, 300, 8, 1.3)
    else:
        if scene == "mixed":
            sc.loadPrims(oracle.OracleScene(accel="None", prims=oracle.synthetic_mixed_prims(40)).prims())
        else:
            n1, r1 = oracle.OracleScene(preset=18, accel="None").nodes()
            n2, r2 = oracle.OracleScene(preset=11, accel="None").nodes()
            nodes = list(n1) + [(t, a + len(n1) if a >= 0 else -1, b + len(n1) if b >= 0 else -1, m, p) for t, a, b, m, p in n2]
            sc.loadNodes(nodes, list(r1) + [r + len(n1) for r in r2])
        pts = np.random.default_rng(7).uniform(-3.3, 3.3, (300, 3)).astype(np.float32)
    ids = check_objects(pctx, octx, pctx.points(pts, normal=False, time=time), time, (scene, accel, "as given"))
    ids |= check_objects(pctx, octx, pctx.points(pts, snap=3, time=time), time, (scene, accel, "projected"))
    assert len(ids - {-1}) >= {"mixed": 10, "forest": 3, 12: 1}[scene], ids


def device_points(rm, ctx, q, d_points, n, position="own", stream=None, want=(1, 1, 1, 1, 1, 1)):
    """rm_scene_points_device through ctypes with guarded buffers -> the six outputs as numpy arrays (None where not asked
    for).  position "alias": d_points is the position buffer."""
    import torch
    N = rm._native
    sizes = (12, 8, 12, 4, 4, 4)
    bufs = [torch.full((n * s + 64,), FILL, dtype=torch.uint8, device="cuda") if w else None for s, w in zip(sizes, want)]
    ptrs = [None if b is None else C.c_void_p(b.data_ptr() + 32) for b in bufs]
    if position == "alias":
        ptrs[0] = C.c_void_p(d_points.data_ptr())
    N.check(ctx._h, N.lib().rm_scene_points_device(ctx._h, C.byref(q), n, C.c_void_p(d_points.data_ptr()), *ptrs,
                                                   None if stream is None else C.c_void_p(stream.cuda_stream)))
    (stream or torch.cuda.current_stream()).synchronize()
    out = []
    for b, s, dt in zip(bufs, sizes, (np.float32, np.float64, np.float32, np.int32, np.int32, np.uint32)):
        if b is None:
            out.append(None)
            continue
        raw = b.cpu().numpy()
        assert (raw[:32] == FILL).all() and (raw[32 + n * s:] == FILL).all(), "written outside the buffer"
        out.append(np.frombuffer(raw[32:32 + n * s].tobytes(), dt))
    if position == "alias":
        out[0] = d_points.cpu().numpy().reshape(-1)
    return out


@pytest.mark.gpu
def test_the_device_entry_equals_the_host_entry(rm, pctx):
    import torch
    N = rm._native
    sc = load(rm, pctx, 3, "BVH")
    sc.camera.setAngles(0.2, 0.5)
    pts = scene_points(rm, 3, 1000, 60, 1.2)
    n = len(pts)
    pctx.scene_set_time(0.25)
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    pctx._attach_diag(acc)
    host = pctx.points(pts, snap=3)
    assert pctx.last_kernel() == "point_kernel<2, 0>"
    flat = [host.position.reshape(-1), host.dist, host.normal.reshape(-1), host.object, host.steps, host.count]
    q = query(rm, snap=3, flags=N.RM_POINT_NORMAL)
    d_pts = torch.from_numpy(pts).cuda()
    for got, w in zip(device_points(rm, pctx, q, d_pts, n), flat):
        assert same_bits(got, w)
    assert same_bits(d_pts.cpu().numpy(), pts)  # the input was left alone
    # a stream of its own; some outputs absent
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d2 = torch.from_numpy(pts).cuda()
        got = device_points(rm, pctx, q, d2, n, stream=st, want=(0, 1, 0, 1, 0, 0))
    assert got[0] is None and same_bits(got[1], host.dist) and same_bits(got[3], host.object) and got[5] is None
    # the positions written over the points
    got = device_points(rm, pctx, q, d_pts, n, position="alias")
    for g, w in zip(got, flat):
        assert same_bits(g, w)
    # the Python method on tensors, and device=True
    r = pctx.points(torch.from_numpy(pts).cuda(), snap=3)
    r2 = pctx.points(pts, snap=3, device=True)
    torch.cuda.synchronize()
    for a, b, w in zip(r, r2, host):
        assert a.is_cuda and same_bits(a.cpu().numpy(), w) and same_bits(b.cpu().numpy(), w)
    # no point: RM_OK, nothing is launched or written
    assert N.lib().rm_scene_points(pctx._h, C.byref(q), 0, None, None, None, None, None, None, None) == N.RM_OK
    assert N.lib().rm_scene_points_device(pctx._h, C.byref(q), 0, None, None, None, None, None, None, None, None) == N.RM_OK
    assert len(pctx.points(np.zeros((0, 3), np.float32)).dist) == 0
    # the `filter` knob changes no bit
    pctx.set_option("filter", 0)
    try:
        other = pctx.points(pts, snap=3)
    finally:
        pctx.set_option("filter", 1)
    for a, w in zip(other, host):
        assert same_bits(a, w)
    # not a render entry: the armed diagnostics are still armed and fire on the next render; the scene's time was kept
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "a point query fired the diagnostics"
    W, H = 64, 48
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    torch.cuda.synchronize()
    s = bufs[2].cpu().numpy().view(np.uint16).astype(np.int64)
    assert pctx.decode_acc(acc)["total_sdf"] == int(s.sum())


@pytest.mark.gpu
def test_the_scene_time_is_kept_and_the_scene_methods_use_their_own(rm, oracle, pctx):
    sc = load(rm, pctx, 12, "None")
    pts = scene_points(rm, 12, 64, 61)
    osc = oracle.OracleScene(preset=12, accel="None")
    sc.updateTime(0.2)
    r = pctx.points(pts, time=0.7)
    assert same_bits(r.dist, M.oracle_distance(osc, 0.7)(pts)[0])
    after, _ = pctx.scene_distance(pts)  # rm_scene_set_time's value was kept
    assert same_bits(after, M.oracle_distance(osc, 0.2)(pts)[0]) and not same_bits(after, r.dist)
    # Scene.getNormal, nearestObject, projectToSurface at the scene's own time
    at02 = pctx.points(pts, time=0.2)
    assert sc.getNormal(pts[5]) == [float(x) for x in at02.normal[5]] and sc.nearestObject(pts[5]) == int(at02.object[5])
    pos, dist, steps = sc.projectToSurface(pts, steps=4, tol=1e-4)
    want = pctx.points(pts, normal=False, object=False, snap=4, time=0.2)
    assert same_bits(pos, want.position) and same_bits(dist, want.dist) and np.array_equal(steps, want.steps)


@pytest.mark.gpu
def test_a_host_batch_crosses_the_chunk_of_the_host_form(rm, pctx):
    """2^22 + 257 points of the Sphere preset, dist and object only: the host form takes 2^22 at a time."""
    import torch
    N = rm._native
    load(rm, pctx, 0, "None")
    chunk, n = 1 << 22, (1 << 22) + 257
    pts = np.random.default_rng(9).uniform(-2.5, 2.5, (n, 3)).astype(np.float32)
    q = query(rm)
    dist = np.full(n, np.nan, np.float64)
    obj = np.full(n, -7, np.int32)
    N.check(pctx._h, N.lib().rm_scene_points(pctx._h, C.byref(q), n, vp(pts), None, vp(dist), None, vp(obj), None, None))
    d_pts = torch.from_numpy(pts).cuda()
    _, d_dist, _, d_obj, _, _ = device_points(rm, pctx, q, d_pts, n, want=(0, 1, 0, 1, 0, 0))
    assert same_bits(dist, d_dist) and same_bits(obj, d_obj)
    assert (obj == 0).all() and (dist < 0).any() and (dist > 0).any()
    for i in (0, chunk - 1, chunk, n - 1):
        r = pctx.points(pts[i:i + 1], normal=False)
        assert same_bits(r.dist, dist[i:i + 1]) and r.object[0] == obj[i], i


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel", [(0, "None"), (3, "BVH")])
def test_mesh_attributes_are_the_model_on_the_plain_vertices(rm, pctx, octx, preset, accel):
    sc = load(rm, pctx, preset, accel)
    mn, mx = root_box(rm, preset)
    m = 0.13 * (mx - mn)
    step = (mx - mn + 2 * m) / 32
    lat = (mn - m, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), (33, 33, 33))
    v0, f0 = pctx.mesh(*lat)
    assert len(v0) > 200 and len(f0) > 200
    v, f, nrm, obj = pctx.mesh(*lat, attributes=True, snap=3)
    assert same_bits(f, f0) and nrm.shape == v.shape == v0.shape and obj.shape == (len(v),) and obj.dtype == np.int32
    want = M.points_model(M.context_distance(pctx), v0, snap=3, tol=1e-4)
    assert same_bits(v, want.position) and same_bits(nrm, want.normal)
    assert (want.steps > 0).any()
    direct = pctx.points(v0, snap=3)
    assert np.array_equal(obj, direct.object)
    check_objects(pctx, octx, direct, 0.0, (preset, accel))
    if preset == 0:
        assert (obj == 0).all()
    else:
        assert len(set(obj.tolist()) - {-1}) >= 10
    # snap = 0 leaves the vertices as they are
    v1, f1, n1, o1 = pctx.mesh(*lat, attributes=True)
    at0 = pctx.points(v0)
    assert same_bits(v1, v0) and same_bits(f1, f0) and same_bits(n1, at0.normal) and np.array_equal(o1, at0.object)
    # triangles, the device form, the scene's own entry
    import torch
    tv, tf, tn, to = pctx.mesh(*lat, attributes=True, snap=3, device=True, triangles=True)
    torch.cuda.synchronize()
    assert same_bits(tv.cpu().numpy(), v) and same_bits(tn.cpu().numpy(), nrm) and same_bits(to.cpu().numpy(), obj) and tuple(tf.shape) == (2 * len(f), 3)
    sv, sf, sn, so = sc.toMesh(*lat, attributes=True, snap=3)
    assert same_bits(sv, v) and same_bits(sf, f) and same_bits(sn, nrm) and same_bits(so, obj)
    assert len(sc.toMesh(*lat)) == 2
