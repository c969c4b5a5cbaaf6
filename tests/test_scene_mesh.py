"""Meshes (rm_mesh_field_device, rm_scene_mesh; Context.mesh, mesh_field, mesh_box, Scene.toMesh, save_obj): naive surface
nets over a lattice of distances, on the device.  CPU tests: the ABI contract on a host-only context, the numpy model of
tests/mesh_model.py against answers worked by hand and against the topology of an analytic sphere and torus, the registers of
the kernels.  GPU tests: the device entry equals the model byte for byte -- vertices, quads and info -- on hand-made volumes of
both value types, with nothing to find, under the capacity protocol and on two streams; rm_scene_mesh equals the model applied
to rm_scene_field's own distances, with the Euler characteristic of the shipped scenes; no side effects; the Python mirror."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_model as FM  # noqa: E402
import mesh_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
FILL = 0xA5
NAN, INF = float("nan"), float("inf")
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
SKEW = ((0.25, -1.5, 0.75), (0.1, 0.013, -0.007), (-0.011, 0.21, 0.017), (0.023, -0.019, 0.37))  # no axis-aligned step, right-handed


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def lattice(rm, origin, du, dv, dw, shape, time=0.0):
    lat = rm._native.rm_lattice()
    for name, v in (("origin", origin), ("du", du), ("dv", dv), ("dw", dw)):
        getattr(lat, name)[:] = [float(x) for x in np.asarray(v, np.float32)]
    lat.nu, lat.nv, lat.nw = shape
    lat.time = time
    return lat


def vectors(lat):
    return tuple(np.array(list(getattr(lat, k)), np.float32) for k in ("origin", "du", "dv", "dw")) + (lat.nu, lat.nv, lat.nw)


def model(lat, values, iso=0.0):
    """-> (vertices, quads, info as the four int64 of rm_mesh_info)"""
    v, q, holes = M.mesh(values, *vectors(lat), iso)
    return v, q, np.array([len(v), len(q), holes, 0], np.int64)


# ----------------------------------------------------------------------------------------------------- CPU: ABI contract

def test_the_library_exports_the_mesh_entries_and_the_record_has_its_size(rm):
    N = rm._native
    for name in ("rm_mesh_field_device", "rm_scene_mesh"):
        assert hasattr(N.lib(), name), name
    assert C.sizeof(N.rm_mesh_info) == 32
    assert [f for f, _ in N.rm_mesh_info._fields_] == ["n_vertices", "n_quads", "n_holes", "reserved"]
    assert (N.RM_MESH_F64, N.RM_MESH_F32) == (0, 1)
    header = open(os.path.join(ROOT, "include", "rm_raymarch.h")).read()
    assert re.search(r"enum\s*\{\s*RM_MESH_F64\s*=\s*0,\s*RM_MESH_F32\s*=\s*1\s*\}", header)


def test_bad_mesh_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    ctx.scene_from_preset(3, 2)
    bare = rm.Context(None)  # no scene
    val = np.zeros(64, np.float64)
    ver, qua = np.zeros(3 * 64, np.float32), np.zeros(4 * 64, np.uint32)
    raw_info = np.zeros(8, np.int64)
    info = N.rm_mesh_info()

    def lat(shape=(4, 4, 4), origin=(0, 0, 0), du=(0.1, 0, 0), dv=(0, 0.1, 0), dw=(0, 0, 0.1), time=0.0, reserved=0):
        l = lattice(rm, origin, du, dv, dw, shape, time)
        l.reserved = reserved
        return l

    def device(c, l, values=vp(val), vt=0, iso=0.0, v=vp(ver), cv=64, q=vp(qua), cq=64, inf=vp(raw_info)):
        return L.rm_mesh_field_device(c._h, None if l is None else C.byref(l), values, vt, iso, v, cv, q, cq, inf, None)

    def scene(c, l, iso=0.0, v=vp(ver), cv=64, q=vp(qua), cq=64, inf=C.byref(info)):
        return L.rm_scene_mesh(c._h, None if l is None else C.byref(l), iso, v, cv, q, cq, inf)

    def both(c, l, **kw):
        kd = dict(kw)
        ks = {k: v for k, v in kw.items() if k not in ("values", "vt")}
        x, y = device(c, l, **kd), scene(c, l, **ks)
        assert x == y, (x, y, kw)
        return x

    # everything rm_scene_field refuses about a lattice, also when another count is 0
    bad = [(dict(shape=(-1, 4, 4)), (1, 2)), (dict(shape=(4, 65536, 4)), (0, 2)), (dict(shape=(4, 4, -7)), (0, 1)), (dict(reserved=1), (0, 1, 2)),
           (dict(origin=(NAN, 0, 0)), (0, 1, 2)), (dict(du=(0, INF, 0)), (0, 1, 2)), (dict(dv=(0, 0, -INF)), (0, 1, 2)),
           (dict(dw=(NAN, 0, 0)), (0, 1, 2)), (dict(time=NAN), (0, 1, 2)), (dict(time=INF), (0, 1, 2)),
           (dict(du=(3e38, 0, 0), shape=(3, 4, 4)), (1, 2)),
           (dict(origin=(-3e38, 0, 0), dw=(-3e38, 0, 0), shape=(4, 4, 2)), (0, 1))]
    for kw, free in bad:
        for c in (ctx, bare):
            assert both(c, lat(**kw)) == N.RM_E_INVALID, kw
        for axis in free:
            shape = list(kw.get("shape", (4, 4, 4)))
            shape[axis] = 0
            assert both(ctx, lat(**dict(kw, shape=tuple(shape)))) == N.RM_E_INVALID, (kw, axis)
    assert both(ctx, None) == N.RM_E_INVALID
    assert both(ctx, lat(shape=(1025, 1024, 1024))) == N.RM_E_INVALID            # 2^30 + 2^20 points
    assert both(ctx, lat(shape=(1024, 1024, 1024), du=(1e-3, 0, 0), dv=(0, 1e-3, 0), dw=(0, 0, 1e-3))) == N.RM_E_NO_DEVICE  # 2^30: allowed
    # the other arguments, on a lattice with cells and on one with a zero count (no cells: still checked)
    for shape in ((4, 4, 4), (4, 0, 4), (1, 4, 4)):
        l = lat(shape=shape)
        cells = min(shape) >= 2
        assert device(ctx, l, values=None) == (N.RM_E_INVALID if cells else N.RM_E_NO_DEVICE), shape
        assert device(ctx, l, inf=None) == N.RM_E_INVALID and scene(ctx, l, inf=None) == N.RM_E_INVALID
        for iso in (NAN, INF, -INF):
            assert both(ctx, l, iso=iso) == N.RM_E_INVALID
        for vt in (-1, 2, 7):
            assert device(ctx, l, vt=vt) == N.RM_E_INVALID
        assert both(ctx, l, cv=-1) == N.RM_E_INVALID and both(ctx, l, cq=-1) == N.RM_E_INVALID
        assert both(ctx, l, v=None) == N.RM_E_INVALID and both(ctx, l, q=None) == N.RM_E_INVALID  # a capacity of 64 without a buffer
        for off in (1, 2):
            assert both(ctx, l, v=C.c_void_p(ver.ctypes.data + off)) == N.RM_E_INVALID
            assert both(ctx, l, q=C.c_void_p(qua.ctypes.data + off)) == N.RM_E_INVALID
            assert both(ctx, l, v=C.c_void_p(ver.ctypes.data + off), cv=0) == N.RM_E_INVALID  # alignment is asked of any pointer given
            assert device(ctx, l, values=C.c_void_p(val.ctypes.data + off), vt=1) == N.RM_E_INVALID
        for off in (1, 2, 4):
            assert device(ctx, l, values=C.c_void_p(val.ctypes.data + off), vt=0) == N.RM_E_INVALID
            assert device(ctx, l, inf=C.c_void_p(raw_info.ctypes.data + off)) == N.RM_E_INVALID
        # well formed: no device
        assert both(ctx, l) == N.RM_E_NO_DEVICE
        assert both(ctx, l, v=None, cv=0, q=None, cq=0) == N.RM_E_NO_DEVICE       # the counting call
        assert device(ctx, l, values=C.c_void_p(val.ctypes.data + 4), vt=1) == N.RM_E_NO_DEVICE
    assert L.rm_mesh_field_device(None, C.byref(lat()), vp(val), 0, 0.0, vp(ver), 64, vp(qua), 64, vp(raw_info), None) == N.RM_E_INVALID
    assert L.rm_scene_mesh(None, C.byref(lat()), 0.0, vp(ver), 64, vp(qua), 64, C.byref(info)) == N.RM_E_INVALID
    # the scene check comes last, and only rm_scene_mesh has one
    assert scene(bare, lat(reserved=1)) == N.RM_E_INVALID and scene(bare, lat(), iso=NAN) == N.RM_E_INVALID
    assert scene(bare, lat()) == N.RM_E_NO_DEVICE and device(bare, lat()) == N.RM_E_NO_DEVICE
    for call in (lambda: ctx.mesh(*UNIT, (4, 4, 4)), lambda: ctx.mesh_field(np.zeros(64), *UNIT, (4, 4, 4))):
        with pytest.raises(rm.RmError) as e:
            call()
        assert e.value.code == N.RM_E_NO_DEVICE


# --------------------------------------------------------------------------------------- CPU: the model, worked by hand

def test_one_inside_corner_gives_one_vertex_at_the_mean_of_three_crossings():
    """2 x 2 x 2 points, point (0, 0, 0) = -1 inside, its neighbours along x, y, z = 3, 1, 7, the rest 1.  The three edges that
    leave the corner cross: t = (0 - (-1)) / (b - (-1)) = 1/4, 1/2, 1/8, at local (1/4, 0, 0), (0, 1/2, 0), (0, 0, 1/8); m = 3, so
    f = (1/12, 1/6, 1/24).  Lattice origin (1, 2, 3), steps 2, 4, 8: the vertex is (1 + 2/12, 2 + 4/6, 3 + 8/24), each formed in
    binary64 as origin + (0 + f) * step and rounded once.  One cell: no quad."""
    val = np.ones((2, 2, 2))
    val[0, 0, 0], val[0, 0, 1], val[0, 1, 0], val[1, 0, 0] = -1, 3, 1, 7
    v, q, holes = M.mesh(val, (1, 2, 3), (2, 0, 0), (0, 4, 0), (0, 0, 8), 2, 2, 2)
    assert v.shape == (1, 3) and v.dtype == np.float32 and q.shape == (0, 4) and q.dtype == np.uint32 and holes == 0
    want = [np.float32(1.0 + ((0.0 + 0.25) / 3.0) * 2.0), np.float32(2.0 + ((0.0 + 0.5) / 3.0) * 4.0), np.float32(3.0 + ((0.0 + 0.125) / 3.0) * 8.0)]
    assert v[0].tolist() == want
    # a count below 2: no cells
    for shape in ((1, 2, 4), (2, 1, 4), (4, 2, 1), (0, 2, 2)):
        vv, qq, hh = M.mesh(np.full(shape[0] * shape[1] * shape[2], -1.0), *UNIT, *shape)
        assert len(vv) == 0 and len(qq) == 0 and hh == 0


def test_a_single_inside_point_gives_the_cube_of_eight_vertices_and_six_quads():
    """3 x 3 x 3 points, 1 outside, the centre (1, 1, 1) = -1: every t is 0.5.  Each of the eight cells has the centre as a
    corner and three crossing edges that end there; cell (i, j, k) (vertex i + 2 j + 4 k) has them at local coordinates 1 - i on
    two axes and 0.5 on the third, so f = (2 (1 - i) + 0.5) / 3 and the vertex lies at 5/6 (low cell) or 1 + 1/6 (high cell)
    per axis.  The six lattice edges at the centre, by key 3 l(p) + A, with c0 .. c3 from the rule:
      p = (1,1,0) A = 2, outside, key 14: c = (0,0,0) (1,0,0) (1,1,0) (0,1,0) -> vertices (0, 1, 3, 2) -> reversed (0, 2, 3, 1)
      p = (1,0,1) A = 1, outside, key 31: c = (0,0,0) (0,0,1) (1,0,1) (1,0,0) -> (0, 4, 5, 1) -> (0, 1, 5, 4)
      p = (0,1,1) A = 0, outside, key 36: c = (0,0,0) (0,1,0) (0,1,1) (0,0,1) -> (0, 2, 6, 4) -> (0, 4, 6, 2)
      p = (1,1,1) A = 0, inside,  key 39: c = (1,0,0) (1,1,0) (1,1,1) (1,0,1) -> (1, 3, 7, 5)
      p = (1,1,1) A = 1, inside,  key 40: c = (0,1,0) (0,1,1) (1,1,1) (1,1,0) -> (2, 6, 7, 3)
      p = (1,1,1) A = 2, inside,  key 41: c = (0,0,1) (1,0,1) (1,1,1) (0,1,1) -> (4, 5, 7, 6)"""
    val = np.ones((3, 3, 3))
    val[1, 1, 1] = -1
    v, q, holes = M.mesh(val, *UNIT, 3, 3, 3)
    assert v.shape == (8, 3) and holes == 0
    lo, hi = np.float32((1.0 + 1.0 + 0.5) / 3.0), np.float32(1.0 + (0.0 + 0.0 + 0.5) / 3.0)
    for n in range(8):
        assert v[n].tolist() == [hi if n & 1 else lo, hi if n & 2 else lo, hi if n & 4 else lo], n
    assert q.tolist() == [[0, 2, 3, 1], [0, 1, 5, 4], [0, 4, 6, 2], [1, 3, 7, 5], [2, 6, 7, 3], [4, 5, 7, 6]]
    # the winding: every normal points away from the inside point
    p = v.astype(np.float64)
    normal = np.cross(p[q[:, 1]] - p[q[:, 0]], p[q[:, 3]] - p[q[:, 0]])
    assert ((normal * (p[q].mean(axis=1) - 1.0)).sum(axis=1) > 0).all()
    assert M.is_closed_manifold(q) and len(v) - len(q) == 2
    # the complement (centre outside) has the same vertices and every quad reversed
    v2, q2, _ = M.mesh(-val, *UNIT, 3, 3, 3)
    assert same_bits(v2, v) and q2.tolist() == [[r[0], r[3], r[2], r[1]] for r in q.tolist()]


def test_values_at_iso_nan_and_infinities():
    def one(corner, others=1.0, iso=0.0, second=None):
        val = np.full((2, 2, 2), others)
        val[0, 0, 0] = corner
        if second is not None:
            val[1, 1, 1] = second
        v, q, holes = M.mesh(val, *UNIT, 2, 2, 2, iso)
        return len(v), holes

    assert one(0.37, iso=0.37) == (0, 0)                                   # equal to iso: outside, like the rest
    assert one(np.nextafter(0.37, 0.0), iso=0.37) == (1, 0)
    assert one(-0.0) == (0, 0) and one(0.0) == (0, 0)                      # -0.0 < 0.0 is false
    assert one(0.37, others=0.0, iso=0.37) == (1, 0)                       # ... and now the corner alone is outside
    assert one(NAN) == (0, 0)                                              # NaN is outside: all outside, not even a hole
    assert one(NAN, others=-1.0) == (0, 1)                                 # mixed with a non-finite corner: a hole
    assert one(-1.0, second=NAN) == (0, 1)
    assert one(-INF) == (0, 1) and one(INF) == (0, 0) and one(INF, others=-1.0) == (0, 1)
    assert one(-1.0, second=INF) == (0, 1)
    # a hole takes its quads with it: the cube of the previous test with one far corner NaN loses a vertex and three quads
    val = np.ones((3, 3, 3))
    val[1, 1, 1] = -1
    val[2, 2, 2] = NAN
    v, q, holes = M.mesh(val, *UNIT, 3, 3, 3)
    assert (len(v), len(q), holes) == (7, 3, 1) and q.tolist() == [[0, 2, 3, 1], [0, 1, 5, 4], [0, 4, 6, 2]]
    # float32 values are widened
    v32, _, _ = M.mesh(np.array([-1, 3, 1, 1, 7, 1, 1, 1], np.float32), *UNIT, 2, 2, 2)
    assert v32[0].tolist() == [np.float32(0.25 / 3.0), np.float32(0.5 / 3.0), np.float32(0.125 / 3.0)]


def test_the_position_rule_on_a_skew_lattice():
    """3 x 3 x 3 points, only point (2, 2, 2) inside (-3 against 1: t = (0 - 1) / (-3 - 1) = 0.25 on the three edges that end
    there): cell (1, 1, 1) alone is active, its crossings at local (0.25, 1, 1), (1, 0.25, 1), (1, 1, 0.25), f = 2.25 / 3 = 0.75
    per axis, fractional index 1.75 each.  Component c = ((o + 1.75 du) + 1.75 dv) + 1.75 dw in binary64 from the binary32
    vectors, left to right, rounded once."""
    val = np.ones((3, 3, 3))
    val[2, 2, 2] = -3
    v, q, holes = M.mesh(val, *SKEW, 3, 3, 3)
    assert v.shape == (1, 3) and len(q) == 0 and holes == 0
    o, du, dv, dw = (np.asarray(x, np.float32) for x in SKEW)
    f = 1.0 + ((0.25 + 1.0) + 1.0) / 3.0
    assert f == 1.75
    for c in range(3):
        want = np.float32(((float(o[c]) + f * float(du[c])) + f * float(dv[c])) + f * float(dw[c]))
        assert v[0, c] == want, c
    # the single rounding is visible: rounding the lattice point and the offset separately differs somewhere
    pts = FM.points(*SKEW, 3, 3, 3).reshape(3, 3, 3, 3)
    apart = pts[1, 1, 1] + np.float32(0.75) * (du + dv + dw)
    assert (apart != v[0]).any()


def analytic(kind, n, half):
    x = np.linspace(-half, half, n)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    if kind == "sphere":
        d = np.sqrt(X * X + Y * Y + Z * Z) - 1.5
    else:
        d = np.sqrt((np.sqrt(X * X + Z * Z) - 1.0) ** 2 + Y * Y) - 0.4
    s = 2.0 * half / (n - 1)
    return d, ((-half,) * 3, (s, 0, 0), (0, s, 0), (0, 0, s))


@pytest.mark.parametrize("kind,n,half,euler", [("sphere", 9, 2.0, 2), ("torus", 17, 1.75, 0)])
def test_the_models_meshes_are_closed_manifolds_of_the_right_genus(kind, n, half, euler):
    d, vecs = analytic(kind, n, half)
    v, q, holes = M.mesh(d, *vecs, n, n, n)
    assert holes == 0 and len(v) - len(q) == euler, (len(v), len(q))
    assert M.is_closed_manifold(q)
    p = v.astype(np.float64)  # outward: the normal agrees with the distance's gradient direction, away from the centre line
    normal = np.cross(p[q[:, 1]] - p[q[:, 0]], p[q[:, 3]] - p[q[:, 0]])
    c = p[q].mean(axis=1)
    if kind == "sphere":
        out = c
    else:
        ring = np.stack([c[:, 0], np.zeros(len(c)), c[:, 2]], axis=1)
        out = c - ring / np.linalg.norm(ring, axis=1, keepdims=True)
    assert ((normal * out).sum(axis=1) > 0).all()


# ------------------------------------------------------------------------------------------------- CPU: build invariants

def test_mesh_kernels_spill_nothing_and_use_no_scratch():
    from test_build_invariants import HIPCC, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage((), "rm_mesh.hip")
    kernels = {n: r for n, r in usage.items() if "mesh_" in n and "_kernel" in n}
    assert len(kernels) == 7, sorted(usage)  # count, vertex and quad for both value types, one scan
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope="module")
def mctx(rm):
    """A context of its own.  Interpreter only, like the field tests': the sampling launch is ahead-of-time."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    return c


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_mesh(rm, ctx, lat, d_values, iso, cap_v, cap_q, stream=None, null_when_empty=True):
    """One rm_mesh_field_device call with every output between guard bytes -> (vertices float32 [cap_v, 3], quads uint32
    [cap_q, 4], info int64 [4]) as raw copies of the buffers' payloads: what lies beyond a total is the fill."""
    import torch
    N = rm._native
    vt = N.RM_MESH_F32 if d_values.dtype == torch.float32 else N.RM_MESH_F64
    bufs = [torch.full((size + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda") for size in (12 * cap_v, 16 * cap_q, 32)]
    ptr = [C.c_void_p(b.data_ptr() + GUARD) for b in bufs]
    if null_when_empty:
        ptr[0], ptr[1] = (ptr[0] if cap_v else None), (ptr[1] if cap_q else None)
    s = None if stream is None else C.c_void_p(stream.cuda_stream)
    N.check(ctx._h, N.lib().rm_mesh_field_device(ctx._h, C.byref(lat), C.c_void_p(d_values.data_ptr()), vt, iso, ptr[0], cap_v, ptr[1], cap_q,
                                                 ptr[2], s))
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    raw = [b.cpu().numpy() for b in bufs]
    for r in raw:
        assert (r[:GUARD] == FILL).all() and (r[len(r) - GUARD:] == FILL).all(), "written outside a buffer"
    pay = [r[GUARD:len(r) - GUARD] for r in raw]
    return pay[0].view(np.float32).reshape(cap_v, 3), pay[1].view(np.uint32).reshape(cap_q, 4), pay[2].view(np.int64)


def full_mesh(rm, ctx, lat, d_values, iso=0.0):
    """The counting call, then the filling call with exact capacities -> (vertices, quads, info)."""
    v0, q0, info = device_mesh(rm, ctx, lat, d_values, iso, 0, 0)
    v, q, info2 = device_mesh(rm, ctx, lat, d_values, iso, int(info[0]), int(info[1]))
    assert np.array_equal(info, info2) and info[3] == 0
    return v, q, info


def assert_equals_model(got, want, what):
    for g, w, name in zip(got, want, ("vertices", "quads", "info")):
        assert g.shape == w.shape and same_bits(g, w), (what, name, g.shape, w.shape, int((np.asarray(g) != np.asarray(w)).sum()) if g.shape == w.shape else None)


def scan_constants():
    text = open(os.path.join(ROOT, "cpu_raymarcher_amd", "csrc", "rm_kernels.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % k, text).group(1)) for k in ("RM_MESH_BLOCK", "RM_MESH_SCAN_STEP"))


VOLUMES = [(2, 2, 2), (2, 2, 70), (65, 3, 3), (19, 13, 7), (97, 61, 45)]
_random = {}


def random_volume(shape, dtype):
    """Random finite values (about half of them inside at iso 0) and their model mesh, made once per (shape, type)."""
    key = (shape, np.dtype(dtype).name)
    if key not in _random:
        rng = np.random.default_rng(1000 + shape[0] * 7 + shape[2])
        val = rng.standard_normal(shape[0] * shape[1] * shape[2]).astype(dtype)
        _random[key] = val
    return _random[key]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", VOLUMES)
def test_the_device_entry_equals_the_model_on_random_volumes(rm, mctx, shape, dtype):
    block, step = scan_constants()
    assert (block, step) == (256, 1024)
    if shape == VOLUMES[-1]:
        # mesh_scan_kernel takes 1024 workgroup totals per step of its loop, a workgroup covers 256 points: this lattice has
        # 1041 workgroups, so the scan carries its sums into a second step
        assert (shape[0] * shape[1] * shape[2] + block - 1) // block == 1041 > step
    lat = lattice(rm, *SKEW, shape)
    val = random_volume(shape, dtype)
    want = model(lat, val)
    assert want[2][0] >= 1 and want[2][2] == 0 and (want[2][1] >= 1 or shape[:2] == (2, 2)), want[2]  # (no edge of a 2 x 2 x n lattice has four cells)
    got = full_mesh(rm, mctx, lat, on_device(val))
    assert_equals_model(got, want, (shape, dtype))
    assert mctx.last_kernel() == "mesh_count_kernel<%s>" % ("float" if dtype == np.float32 else "double")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_values_at_iso_nan_and_infinities_on_the_device(rm, mctx, dtype):
    shape = (19, 13, 7)
    iso = float(np.float32(0.37))  # a binary32 value, so that both value types hold it exactly
    rng = np.random.default_rng(77)
    val = (rng.standard_normal(19 * 13 * 7) * 0.5 + 0.37).astype(dtype)
    pick = rng.permutation(len(val))
    val[pick[:60]] = iso
    val[pick[60:75]] = NAN
    val[pick[75:85]] = INF
    val[pick[85:95]] = -INF
    lat = lattice(rm, *SKEW, shape)
    want = model(lat, val, iso)
    assert want[2][2] > 20 and want[2][0] > 100 and want[2][1] > 50, want[2]
    assert_equals_model(full_mesh(rm, mctx, lat, on_device(val), iso), want, dtype)
    # the values at iso are outside: moving them just below changes the mesh
    below = val.copy()
    below[pick[:60]] = np.nextafter(dtype(iso), dtype(0))
    assert not same_bits(model(lat, below, iso)[2], want[2]) or not same_bits(model(lat, below, iso)[1], want[1])
    assert_equals_model(full_mesh(rm, mctx, lat, on_device(below), iso), model(lat, below, iso), (dtype, "below"))


@pytest.mark.gpu
def test_a_volume_without_a_surface(rm, mctx):
    import torch
    N = rm._native
    lat = lattice(rm, *SKEW, (19, 13, 7))
    n = 19 * 13 * 7
    for value in (1.0, -1.0):
        v, q, info = device_mesh(rm, mctx, lat, on_device(np.full(n, value)), 0.0, 32, 32)  # capacities above the totals
        assert info.tolist() == [0, 0, 0, 0]
        assert (v.view(np.uint8) == FILL).all() and (q.view(np.uint8) == FILL).all()
    # all NaN: outside everywhere, not even a hole
    assert device_mesh(rm, mctx, lat, on_device(np.full(n, NAN)), 0.0, 32, 32)[2].tolist() == [0, 0, 0, 0]
    # lattices without a cell: zero totals, nothing launched, null values allowed
    mctx.scene_from_preset(0, 0)
    before = mctx.last_kernel()
    for shape in ((1, 13, 7), (19, 0, 7), (19, 13, 1)):
        flat = lattice(rm, *SKEW, shape)
        info = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        N.check(mctx._h, N.lib().rm_mesh_field_device(mctx._h, C.byref(flat), None, 0, 0.0, None, 0, None, 0, C.c_void_p(info.data_ptr()), None))
        torch.cuda.synchronize()
        assert info.cpu().tolist() == [0, 0, 0, 0]
        host = N.rm_mesh_info(7, 7, 7, 7)
        N.check(mctx._h, N.lib().rm_scene_mesh(mctx._h, C.byref(flat), 0.0, None, 0, None, 0, C.byref(host)))
        assert (host.n_vertices, host.n_quads, host.n_holes, host.reserved) == (0, 0, 0, 0)
    assert mctx.last_kernel() == before


@pytest.mark.gpu
def test_the_capacity_protocol(rm, mctx):
    shape = (19, 13, 7)
    lat = lattice(rm, *SKEW, shape)
    val = random_volume(shape, np.float64)
    d_val = on_device(val)
    want_v, want_q, want_info = model(lat, val)
    V, Q = int(want_info[0]), int(want_info[1])
    assert V > 40 and Q > 40
    # the counting call: null buffers, and buffers given with a capacity of 0 -- nothing is written either way
    for null in (True, False):
        v, q, info = device_mesh(rm, mctx, lat, d_val, 0.0, 0, 0, null_when_empty=null)
        assert same_bits(info, want_info)
    for cap_v, cap_q in ((V - 1, Q - 1), (1, 1), (V, 1), (1, Q), (0, Q), (V, 0), (V + 5, Q + 5)):
        # nothing at or beyond a capacity (the guards), nothing beyond a total (the fill)
        v, q, info = device_mesh(rm, mctx, lat, d_val, 0.0, cap_v, cap_q)
        assert same_bits(info, want_info), (cap_v, cap_q)
        nv, nq = min(cap_v, V), min(cap_q, Q)
        assert same_bits(v[:nv], want_v[:nv]) and same_bits(q[:nq], want_q[:nq]), (cap_v, cap_q)
        assert (v[nv:].view(np.uint8) == FILL).all() and (q[nq:].view(np.uint8) == FILL).all(), (cap_v, cap_q)
    # a truncated quad list names vertices beyond the vertex capacity
    assert want_q[:Q - 1].max() >= 1


@pytest.mark.gpu
def test_two_calls_on_two_streams_return_identical_bytes(rm, mctx):
    import torch
    N = rm._native
    shape = (97, 61, 45)
    lat = lattice(rm, *SKEW, shape)
    val = random_volume(shape, np.float32)
    d_val = on_device(val)
    want = model(lat, val)
    V, Q = int(want[2][0]), int(want[2][1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for st in streams:  # both enqueued before either is waited for: the entry orders the users of its scratch itself
        with torch.cuda.stream(st):
            v = torch.full((V, 3), -1.0, dtype=torch.float32, device="cuda")
            q = torch.full((Q, 4), -1, dtype=torch.int32, device="cuda")
            info = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        st.synchronize()
        outs.append((v, q, info))
    for st, (v, q, info) in zip(streams, outs):
        N.check(mctx._h, N.lib().rm_mesh_field_device(mctx._h, C.byref(lat), C.c_void_p(d_val.data_ptr()), N.RM_MESH_F32, 0.0, C.c_void_p(v.data_ptr()), V,
                                                      C.c_void_p(q.data_ptr()), Q, C.c_void_p(info.data_ptr()), C.c_void_p(st.cuda_stream)))
    for st in streams:
        st.synchronize()
    a, b = [[t.cpu().numpy() for t in o] for o in outs]
    for x, y, w in zip(a, b, want):
        assert same_bits(x, y) and same_bits(x, w)


def scene_field(rm, ctx, lat):
    N = rm._native
    dist = np.zeros(lat.nu * lat.nv * lat.nw, np.float64)
    N.check(ctx._h, N.lib().rm_scene_field(ctx._h, C.byref(lat), vp(dist), None, None))
    return dist


def scene_mesh(rm, ctx, lat, iso=0.0):
    """rm_scene_mesh: the counting call, then the filling call between guard bytes -> (vertices, quads, info)."""
    N = rm._native
    info = N.rm_mesh_info(-1, -1, -1, -1)
    N.check(ctx._h, N.lib().rm_scene_mesh(ctx._h, C.byref(lat), iso, None, 0, None, 0, C.byref(info)))
    V, Q = info.n_vertices, info.n_quads
    raw_v, raw_q = np.full(12 * V + 2 * GUARD, FILL, np.uint8), np.full(16 * Q + 2 * GUARD, FILL, np.uint8)
    info2 = N.rm_mesh_info(-1, -1, -1, -1)
    N.check(ctx._h, N.lib().rm_scene_mesh(ctx._h, C.byref(lat), iso, C.c_void_p(raw_v.ctypes.data + GUARD), V + 3, C.c_void_p(raw_q.ctypes.data + GUARD),
                                          Q + 3, C.byref(info2)))  # capacities above the totals: nothing beyond the totals is written
    assert bytes(info) == bytes(info2)
    for r in (raw_v, raw_q):
        assert (r[:GUARD] == FILL).all() and (r[len(r) - GUARD:] == FILL).all(), "written outside a buffer"
    return (raw_v[GUARD:GUARD + 12 * V].view(np.float32).reshape(V, 3), raw_q[GUARD:GUARD + 16 * Q].view(np.uint32).reshape(Q, 4),
            np.frombuffer(bytes(info), np.int64))


def cube_lattice(rm, half, n, time=0.0):
    s = 2.0 * half / (n - 1)
    return lattice(rm, (-half,) * 3, (s, 0, 0), (0, s, 0), (0, 0, s), (n, n, n), time)


def skew_scene_lattice(rm):
    """21 x 19 x 17 points around the origin, 1.9 to either side along every index, no axis-aligned step."""
    du, dv, dw = np.array([0.19, 0.011, -0.006]), np.array([-0.009, 0.211, 0.013]), np.array([0.012, -0.008, 0.2375])
    return lattice(rm, -(10 * du + 9 * dv + 8 * dw), du, dv, dw, (21, 19, 17))


# (preset, acceleration, the lattice, V - Q or None)
SCENE_CASES = {
    "sphere": (0, "None", lambda rm: cube_lattice(rm, 2.0, 17), 2),
    "grid-bvh": (3, "BVH", lambda rm: cube_lattice(rm, 2.0, 17), None),
    "grid-octree": (3, "Octree", lambda rm: cube_lattice(rm, 2.0, 17), None),
    "torus": (5, "None", lambda rm: cube_lattice(rm, 2.0, 17), 0),
    "cube-faces-on-points": (7, "None", lambda rm: cube_lattice(rm, 1.5, 7), 2),
    "animated": (12, "None", lambda rm: cube_lattice(rm, 2.0, 17, time=0.7), None),
    "skew": (0, "None", skew_scene_lattice, 2),
    "nine-spheres": (2, "None", lambda rm: lattice(rm, (-1.6, -1.6, -0.6), (0.1, 0, 0), (0, 0.1, 0), (0, 0, 0.1), (33, 33, 13)), 18),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SCENE_CASES))
def test_the_scene_mesh_equals_the_model_on_the_scenes_own_field(rm, mctx, case):
    preset, accel, make, euler = SCENE_CASES[case]
    rm.Scene(accel, ctx=mctx).loadPreset(preset)
    lat = make(rm)
    mctx.scene_set_time(0.2)
    dist = scene_field(rm, mctx, lat)
    want = model(lat, dist)
    assert want[2][0] > 0 and want[2][1] > 0 and want[2][2] == 0, want[2]
    got = scene_mesh(rm, mctx, lat)
    assert_equals_model(got, want, case)
    assert mctx.last_kernel() == "mesh_count_kernel<double>"
    if euler is not None:
        assert int(got[2][0] - got[2][1]) == euler and M.is_closed_manifold(got[1]), (case, got[2])
    if case == "cube-faces-on-points":
        assert (dist == 0.0).sum() >= 50  # lattice points lie exactly on the faces: a value equal to iso is outside
    if case == "animated":
        # the lattice's time rules (the mesh at the context's time differs) and the context's value is kept
        other = lattice(rm, *[list(getattr(lat, k)) for k in ("origin", "du", "dv", "dw")], (lat.nu, lat.nv, lat.nw), time=0.2)
        assert not same_bits(scene_field(rm, mctx, other), dist)
        pts = FM.points(*vectors(lat))[:64]
        after, _ = mctx.scene_distance(pts)
        assert same_bits(after, scene_field(rm, mctx, other)[:64]) and not same_bits(after, dist[:64])
    if case == "sphere":
        # an offset surface, and the device entry on the resident float32 volume of the same lattice
        assert_equals_model(scene_mesh(rm, mctx, lat, 0.3), model(lat, dist, 0.3), "iso 0.3")
        vol, _ = mctx.field(*[list(getattr(lat, k)) for k in ("origin", "du", "dv", "dw")], shape=(17, 17, 17), dist32=True, count=False, device=True)
        assert_equals_model(full_mesh(rm, mctx, lat, vol), model(lat, dist.astype(np.float32)), "dist32")


@pytest.mark.gpu
def test_mesh_entries_leave_armed_diagnostics_alone(rm, mctx):
    import torch
    W, H = 64, 48
    sc = rm.Scene("BVH", ctx=mctx)
    sc.loadPreset(3)
    sc.camera.setAngles(0.2, 0.5)
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    mctx._attach_diag(acc)
    lat = cube_lattice(rm, 2.0, 17)
    scene_mesh(rm, mctx, lat)
    full_mesh(rm, mctx, lat, on_device(scene_field(rm, mctx, lat)))
    mctx.mesh_box((16, 16, 16))
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "a mesh entry fired the diagnostics"
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    torch.cuda.synchronize()
    got = mctx.decode_acc(acc)  # the armed accumulator was still there for the render
    s = bufs[2].cpu().numpy().view(np.uint16).astype(np.int64)
    i = bufs[3].cpu().numpy().view(np.uint16).astype(np.int64)
    assert got == {"total_sdf": int(s.sum()), "total_iters": int(i.sum()), "max_sdf": int(s.max()), "min_sdf": int(s.min())}


def parse_obj(path):
    v, f = [], []
    for line in open(path):
        t = line.split()
        if t and t[0] == "v":
            v.append([float(x) for x in t[1:]])
        elif t and t[0] == "f":
            f.append([int(x) - 1 for x in t[1:]])
    return np.array(v, np.float32).reshape(-1, 3), np.array(f, np.uint32)


@pytest.mark.gpu
def test_the_python_mirror(rm, mctx, tmp_path):
    import torch
    sc = rm.Scene("None", ctx=mctx)
    sc.loadPreset(5)
    lat = cube_lattice(rm, 2.0, 17)
    vecs = [np.array(list(getattr(lat, k)), np.float32) for k in ("origin", "du", "dv", "dw")]
    want_v, want_q, want_info = scene_mesh(rm, mctx, lat)
    v, q = mctx.mesh(*vecs, (17, 17, 17))
    assert v.dtype == np.float32 and q.dtype == np.uint32 and same_bits(v, want_v) and same_bits(q, want_q)
    # Context.mesh is the two-call sequence of the device entry on the resident volume
    vol, _ = mctx.field(*vecs, shape=(17, 17, 17), count=False, device=True)
    dv_, dq_, _ = full_mesh(rm, mctx, lat, vol)
    assert same_bits(v, dv_) and same_bits(q, dq_)
    # triangles: (0, 1, 2), (0, 2, 3) per quad
    v3, t = mctx.mesh(*vecs, (17, 17, 17), triangles=True)
    assert same_bits(v3, v) and t.shape == (2 * len(q), 3) and t.dtype == np.uint32
    assert np.array_equal(t[0::2], q[:, [0, 1, 2]]) and np.array_equal(t[1::2], q[:, [0, 2, 3]])
    # a left-handed lattice (du and dv exchanged, the values transposed with them) returns the flipped winding
    left = (vecs[0], vecs[2], vecs[1], vecs[3])
    lv, lq = mctx.mesh(*left, (17, 17, 17))
    m_v, m_q, _ = M.mesh(scene_field(rm, mctx, lattice(rm, *left, (17, 17, 17))), *left, 17, 17, 17)
    assert same_bits(lv, m_v) and np.array_equal(lq, m_q[:, [0, 3, 2, 1]])
    p = lv.astype(np.float64)  # ... so its normals point out of the torus like the right-handed ones
    pr = v.astype(np.float64)
    # six times the signed volume of the triangulated surface: positive when the faces are wound outwards
    vol6 = lambda pts, quads: sum(np.einsum("ij,ij->i", pts[quads[:, 0]], np.cross(pts[quads[:, a]], pts[quads[:, b]])).sum() for a, b in ((1, 2), (2, 3)))  # noqa: E731
    assert vol6(pr, q.astype(np.int64)) > 0 and vol6(p, lq.astype(np.int64)) > 0
    # mesh_field: a device tensor (float32 too) and a numpy array
    host = vol.cpu().numpy()
    for values in (vol, host, vol.to(torch.float32), host.astype(np.float32).reshape(-1)):
        fv, fq = mctx.mesh_field(values, *vecs, (17, 17, 17))
        f32 = "float32" in str(values.dtype)
        w = M.mesh(host.astype(np.float32) if f32 else host, *vecs, 17, 17, 17)
        assert same_bits(fv, w[0]) and same_bits(fq, w[1])
    tv, tq = mctx.mesh_field(vol, *vecs, (17, 17, 17), device=True)
    assert tv.is_cuda and tq.is_cuda and tq.dtype == torch.int32 and same_bits(tv.cpu().numpy(), v) and same_bits(tq.cpu().numpy(), q)
    # mesh_box and Scene.toMesh: the torus over its root box, at the scene's time
    sc.updateTime(0.0)
    bv, bq = mctx.mesh_box((24, 24, 24), box=((-2, -2, -2), (2, 2, 2)))
    assert len(bv) - len(bq) == 0 and M.is_closed_manifold(bq)
    ev, eq = sc.toMesh(*vecs, shape=(17, 17, 17))
    assert same_bits(ev, v) and same_bits(eq, q)
    with_box = rm.Scene("BVH", ctx=mctx)  # a scene with a structure reports its root box
    with_box.loadPreset(5)
    sv, sq = with_box.toMesh(cells=(24, 24, 24))
    assert len(sv) - len(sq) == 0 and M.is_closed_manifold(sq)
    # save_obj round-trips
    path = str(tmp_path / "torus.obj")
    rm.save_obj(path, v, q)
    ov, of = parse_obj(path)
    assert same_bits(ov, v) and np.array_equal(of, q)
    rm.save_obj(path, v, t)
    ov, of = parse_obj(path)
    assert same_bits(ov, v) and np.array_equal(of, t)
