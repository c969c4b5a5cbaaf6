"""Field queries (rm_scene_field / rm_scene_field_device, rm_lattice_points, rm_shade_field / rm_shade_field_device;
Context.field, field_slice, lattice_points, shade_field, Scene.distanceField): Scene.getDistance at the points of a lattice the
device forms itself, and the slice image of the result.  CPU tests: the ABI contract on a host-only context, rm_lattice_points
against the numpy model of tests/field_model.py, the model against answers worked by hand, the registers of every
field_kernel instantiation.  GPU tests: the field is rm_scene_distance at rm_lattice_points and the CPU oracle at the model's
points, bit for bit, in both vec3.length builds, at the lattice's own time, for a run-time compiled scene, with absent
outputs, through both entries and across a chunk of the host path; the shade kernel against the model; no side effects."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_model as M  # noqa: E402

GUARD = 64
FILL = 0xA5
NAN, INF = float("nan"), float("inf")


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


def points_of(rm, lat, first=0, n=None):
    total = lat.nu * lat.nv * lat.nw
    n = total - first if n is None else n
    out = np.full((n, 3), 7.0, np.float32)
    assert rm._native.lib().rm_lattice_points(C.byref(lat), first, n, vp(out)) == rm._native.RM_OK
    return out


def shade_args(rm, map=0, range=2.0, band=0.25, line=0.02, lo=0, hi=0, reserved=0):
    sh = rm._native.rm_field_shade()
    sh.map, sh.reserved, sh.range, sh.band, sh.line, sh.lo, sh.hi = map, reserved, range, band, line, lo, hi
    return sh


SKEW = ((0.25, -1.5, 0.75), (0.1, 0.013, -0.007), (-0.011, 0.21, 0.017), (0.023, -0.019, 0.37))  # no axis-aligned step


# ----------------------------------------------------------------------------------------------------- CPU: ABI contract

def test_the_library_exports_the_field_entries_and_the_records_have_their_sizes(rm):
    N = rm._native
    for name in ("rm_scene_field", "rm_scene_field_device", "rm_lattice_points", "rm_shade_field", "rm_shade_field_device"):
        assert hasattr(N.lib(), name), name
    assert C.sizeof(N.rm_lattice) == 72 and C.sizeof(N.rm_field_shade) == 40
    assert N.rm_lattice.time.offset == 64 and N.rm_field_shade.lo.offset == 32
    assert N.FIELD_MAPS == {"distance": 0, "count": 1}


def test_bad_field_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    ctx.scene_from_preset(3, 2)
    dist, d32, cnt = np.zeros(64, np.float64), np.zeros(64, np.float32), np.zeros(64, np.uint32)

    def both(lat, a, b, c):
        ref = None if lat is None else C.byref(lat)
        x = L.rm_scene_field(ctx._h, ref, a, b, c)
        y = L.rm_scene_field_device(ctx._h, ref, a, b, c, None)
        assert x == y, (x, y)
        return x

    def lat(shape=(4, 4, 4), origin=(0, 0, 0), du=(0.1, 0, 0), dv=(0, 0.1, 0), dw=(0, 0, 0.1), time=0.0, reserved=0):
        l = lattice(rm, origin, du, dv, dw, shape, time)
        l.reserved = reserved
        return l

    out = (vp(dist), vp(d32), vp(cnt))
    # (what is wrong, the axes whose count the fault does not depend on)
    bad = [(dict(shape=(-1, 4, 4)), (1, 2)), (dict(shape=(4, 65536, 4)), (0, 2)), (dict(shape=(4, 4, -7)), (0, 1)), (dict(reserved=1), (0, 1, 2)),
           (dict(origin=(NAN, 0, 0)), (0, 1, 2)), (dict(du=(0, INF, 0)), (0, 1, 2)), (dict(dv=(0, 0, -INF)), (0, 1, 2)),
           (dict(dw=(NAN, 0, 0)), (0, 1, 2)), (dict(time=NAN), (0, 1, 2)), (dict(time=INF), (0, 1, 2)),
           (dict(du=(3e38, 0, 0), shape=(3, 4, 4)), (1, 2)),                      # the far corner overflows binary32
           (dict(origin=(-3e38, 0, 0), dw=(-3e38, 0, 0), shape=(4, 4, 2)), (0, 1))]
    for kw, free in bad:
        assert both(lat(**kw), *out) == N.RM_E_INVALID, kw
        for axis in free:  # validation comes first, also when a count is 0 (n = 0)
            shape = list(kw.get("shape", (4, 4, 4)))
            shape[axis] = 0
            assert both(lat(**dict(kw, shape=tuple(shape))), *out) == N.RM_E_INVALID, (kw, axis)
    assert both(None, *out) == N.RM_E_INVALID
    assert both(lat(), None, None, None) == N.RM_E_INVALID                      # nothing asked for
    assert both(lat(shape=(4, 0, 4)), None, None, None) == N.RM_E_NO_DEVICE     # ... of no point: well formed
    for off in (1, 2, 4):
        assert both(lat(), C.c_void_p(dist.ctypes.data + off), None, None) == N.RM_E_INVALID
    for off in (1, 2):
        assert both(lat(), None, C.c_void_p(d32.ctypes.data + off), None) == N.RM_E_INVALID
        assert both(lat(), None, None, C.c_void_p(cnt.ctypes.data + off)) == N.RM_E_INVALID
    assert L.rm_scene_field(None, C.byref(lat()), *out) == N.RM_E_INVALID
    assert L.rm_scene_field_device(None, C.byref(lat()), *out, None) == N.RM_E_INVALID
    # well-formed calls on a host-only context: no device
    assert both(lat(), *out) == N.RM_E_NO_DEVICE
    assert both(lat(), None, vp(d32), None) == N.RM_E_NO_DEVICE
    assert both(lat(shape=(0, 0, 0)), *out) == N.RM_E_NO_DEVICE
    assert both(lat(shape=(65535, 1, 1), du=(1e30, 0, 0)), *out) == N.RM_E_NO_DEVICE  # 6.5e34 is a finite binary32
    with pytest.raises(rm.RmError) as e:
        ctx.field((0, 0, 0), (1, 0, 0), (0, 1, 0), shape=(4, 4))
    assert e.value.code == N.RM_E_NO_DEVICE
    bare = rm.Context(None)  # and the scene check comes last
    assert L.rm_scene_field(bare._h, C.byref(lat(reserved=1)), *out) == N.RM_E_INVALID
    assert L.rm_scene_field(bare._h, C.byref(lat()), *out) == N.RM_E_NO_DEVICE


def test_bad_shade_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)  # no scene: the entry never asks for one
    val = np.zeros(16, np.float64)
    rgba = np.zeros(64, np.uint8)

    def both(sh, n, v, out):
        ref = None if sh is None else C.byref(sh)
        x = L.rm_shade_field(ctx._h, ref, n, v, out)
        y = L.rm_shade_field_device(ctx._h, ref, n, v, out, None)
        assert x == y, (x, y)
        return x

    for n in (8, 0):
        assert both(None, n, vp(val), vp(rgba)) == N.RM_E_INVALID
        assert both(shade_args(rm), n, None, vp(rgba)) == N.RM_E_INVALID
        assert both(shade_args(rm), n, vp(val), None) == N.RM_E_INVALID
        for kw in (dict(map=-1), dict(map=2), dict(reserved=1), dict(range=0.0), dict(range=-1.0), dict(range=NAN), dict(range=INF),
                   dict(band=0.0), dict(band=-0.25), dict(band=NAN), dict(band=INF), dict(line=-0.01), dict(line=NAN), dict(line=INF),
                   dict(map=1, lo=5, hi=4), dict(map=1, reserved=2)):
            assert both(shade_args(rm, **kw), n, vp(val), vp(rgba)) == N.RM_E_INVALID, kw
        assert both(shade_args(rm), n, C.c_void_p(val.ctypes.data + 4), vp(rgba)) == N.RM_E_INVALID
        assert both(shade_args(rm, map=1), n, C.c_void_p(val.ctypes.data + 2), vp(rgba)) == N.RM_E_INVALID
    assert both(shade_args(rm), -1, vp(val), vp(rgba)) == N.RM_E_INVALID
    assert L.rm_shade_field(None, C.byref(shade_args(rm)), 8, vp(val), vp(rgba)) == N.RM_E_INVALID
    # well-formed calls: no device.  COUNT ignores the distance fields, DISTANCE ignores lo and hi; line = 0 is allowed
    assert both(shade_args(rm), 8, vp(val), vp(rgba)) == N.RM_E_NO_DEVICE
    assert both(shade_args(rm, line=0.0, lo=9, hi=1), 8, vp(val), vp(rgba)) == N.RM_E_NO_DEVICE
    assert both(shade_args(rm, map=1, range=NAN, band=-1.0, line=-1.0, lo=3, hi=3), 8, C.c_void_p(val.ctypes.data + 4), vp(rgba)) == N.RM_E_NO_DEVICE
    assert both(shade_args(rm), 0, vp(val), vp(rgba)) == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.shade_field(val)
    assert e.value.code == N.RM_E_NO_DEVICE


# ------------------------------------------------------------------------------------------------- CPU: the lattice's points

@pytest.mark.parametrize("shape", [(19, 13, 3), (1, 1, 1), (1, 70, 1), (65535, 1, 1)])
def test_lattice_points_equal_the_model_byte_for_byte(rm, shape):
    N = rm._native
    cases = [SKEW, ((0, 0, 0), (np.float32(0.1), 0, 0), (0, np.float32(0.1), 0), (0, 0, np.float32(0.1))),
             ((1e-3, 1e3, -7.25), (1.1e-4, 3.3, 0.7), (0.9, -2.9e-5, 1e-7), (1e-8, 0.3, -1.7))]
    for vecs in cases:
        lat = lattice(rm, *vecs, shape)
        got = points_of(rm, lat)
        want = M.points(*vectors(lat))
        assert same_bits(got, want), (shape, vecs, int((got != want).sum()))
    # the binary64 sum of the 0.1f steps is not a binary32 value: the single rounding is visible
    lat = lattice(rm, *cases[1], shape)
    i = np.arange(shape[0], dtype=np.float64)
    exact = i * np.float64(np.float32(0.1))
    if shape[0] > 3:
        assert (exact.astype(np.float32).astype(np.float64) != exact).sum() > shape[0] // 2
        acc = np.cumsum(np.full(shape[0] - 1, np.float32(0.1), np.float32), dtype=np.float32)  # what float32 accumulation would give
        assert (points_of(rm, lat)[1:shape[0], 0] != acc).any()


def test_lattice_point_ranges_and_their_checks(rm):
    N = rm._native
    L = N.lib()
    lat = lattice(rm, *SKEW, (19, 13, 3))
    total = 19 * 13 * 3
    want = M.points(*vectors(lat))
    for first, n in ((0, total), (5, 7), (17, 40), (19 * 13 - 3, 11), (total - 1, 1), (total, 0), (0, 0), (300, 441)):
        raw = np.full(3 * n + 2 * GUARD, 7.0, np.float32)
        assert L.rm_lattice_points(C.byref(lat), first, n, C.c_void_p(raw.ctypes.data + 4 * GUARD)) == N.RM_OK
        assert (raw[:GUARD] == 7.0).all() and (raw[GUARD + 3 * n:] == 7.0).all()
        assert same_bits(raw[GUARD:GUARD + 3 * n], want[first:first + n]), (first, n)
        assert same_bits(M.points(*vectors(lat), first, n), want[first:first + n])
    buf = np.zeros((total, 3), np.float32)
    for first, n in ((-1, 1), (0, -1), (0, total + 1), (total, 1), (total + 1, 0), (5, total - 4), (2 ** 62, 2 ** 62)):
        assert L.rm_lattice_points(C.byref(lat), first, n, vp(buf)) == N.RM_E_INVALID, (first, n)
    assert L.rm_lattice_points(C.byref(lat), 0, 1, None) == N.RM_E_INVALID
    assert L.rm_lattice_points(C.byref(lat), 3, 0, None) == N.RM_OK
    assert L.rm_lattice_points(None, 0, 0, vp(buf)) == N.RM_E_INVALID
    bad = lattice(rm, *SKEW, (19, 13, 3))
    bad.reserved = 1
    assert L.rm_lattice_points(C.byref(bad), 0, 1, vp(buf)) == N.RM_E_INVALID
    empty = lattice(rm, *SKEW, (19, 0, 3))
    assert L.rm_lattice_points(C.byref(empty), 0, 0, None) == N.RM_OK and L.rm_lattice_points(C.byref(empty), 0, 1, vp(buf)) == N.RM_E_INVALID
    assert rm.Context(None).lattice_points(*SKEW, shape=(19, 13, 3)).shape == (3, 13, 19, 3)
    assert same_bits(rm.Context(None).lattice_points(*SKEW, shape=(19, 13, 3)), want)
    assert rm.Context(None).lattice_points(SKEW[0], SKEW[1], SKEW[2], shape=(19, 13)).shape == (1, 13, 19, 3)


def test_the_models_points_for_one_small_lattice_worked_by_hand():
    """origin (1, 2, 3), du = (0.5, 0, 0.1f), dv = (0, 0.25, 0), dw = (0, 0, 2), 4 x 3 x 2 points.
    index 0 = (0, 0, 0): the origin.  index 23 = (3, 2, 1): x = 1 + 3 * 0.5 = 2.5, y = 2 + 2 * 0.25 = 2.5,
    z = (3 + 3 * 0.1f) + 2: 0.1f = 13421773 * 2^-27, three of them 40265319 * 2^-27 = 0.300000004470348358154296875 exactly,
    z = 5.300000004470348358154296875 in binary64 (it needs 29 bits).  binary32 near 5.3 has steps of 2^-21 = 4.76837e-7:
    5.3 = 11114905.6 * 2^-21, so the neighbours are 11114905 * 2^-21 = 5.29999971389770508 and 11114906 * 2^-21 =
    5.30000019073486328; the sum lies 0.61 of a step above the first and rounds to the second.
    index 6 = (2, 1, 0): x = 2, y = 2.25, z = 3 + 2 * 0.1f = 3.2000000029802322 -> steps of 2^-22 = 2.38419e-7 there:
    3.2 = 13421772.8 * 2^-22; the sum is 13421772.8125 * 2^-22 and rounds to 13421773 * 2^-22 = 3.20000004768371582."""
    p = M.points((1, 2, 3), (0.5, 0, np.float32(0.1)), (0, 0.25, 0), (0, 0, 2), 4, 3, 2)
    assert p.shape == (24, 3) and p.dtype == np.float32
    assert p[0].tolist() == [1.0, 2.0, 3.0]
    assert p[23].tolist() == [2.5, 2.5, 11114906 * 2.0 ** -21]
    assert p[6].tolist() == [2.0, 2.25, 13421773 * 2.0 ** -22]
    i, j, k = M.indices(4, 3, 2, 5, 4)
    assert i.tolist() == [1, 2, 3, 0] and j.tolist() == [1, 1, 1, 2] and k.tolist() == [0, 0, 0, 0]
    assert [x.tolist() for x in M.indices(4, 3, 2, 23, 1)] == [[3], [2], [1]]


# ------------------------------------------------------------------------------------------------- CPU: the colour rules

BELOW = lambda x: float(np.nextafter(np.float64(x), 0.0))  # noqa: E731
# (value, pixel with range 2, band 0.25, line 0.02), each worked through the six steps of the header
HAND_DISTANCE = [
    (NAN, (255, 0, 255, 255)),
    (0.0, (255, 255, 255, 255)), (-0.0, (255, 255, 255, 255)),       # |d| < line
    (INF, (230, 140, 50, 255)), (-INF, (60, 120, 230, 255)),          # s = 255: I = 255; y is not below 2^31: q = 0
    (0.02, (87, 53, 19, 255)),                                        # exactly at line: not white; s = (int)2.55 = 2, I = 97, q = 0
    (BELOW(0.02), (255, 255, 255, 255)),
    (2.0, (230, 140, 50, 255)), (-2.0, (60, 120, 230, 255)),          # exactly at range: x = 1, I = 255; q = 8, even
    (BELOW(2.0), (171, 104, 37, 255)),                                # s = 254, I = 254; q = 7, odd: I = 190
    (0.75, (104, 63, 22, 255)), (-0.75, (27, 54, 104, 255)),          # 3 * band: s = (int)95.625 = 95, I = 155; q = 3, odd: I = 116
    (BELOW(0.75), (139, 85, 30, 255)),                                # q = 2, even: I = 155
    (2.0 ** 31 * 0.25, (230, 140, 50, 255)),                          # y = 2^31: q = 0, I = 255
    (2.0 ** 31 * 0.25 - 0.25, (172, 104, 37, 255)),                   # y = 2^31 - 1, odd: I = 191
]
# with line = 0 nothing is white and -0.0 is outside like +0.0: s = 0, I = 96
HAND_NO_LINE = [(0.0, (86, 52, 18, 255)), (-0.0, (86, 52, 18, 255)), (-1e-300, (22, 45, 86, 255))]
# (value, pixel with lo 3, hi 10): s = 0 up to lo, 255 from hi, (v - 3) * 255 // 7 between
HAND_COUNT = [(0, (0, 255, 0, 255)), (3, (0, 255, 0, 255)), (4, (72, 255, 0, 255)), (7, (255, 222, 0, 255)), (9, (255, 76, 0, 255)),
              (10, (255, 2, 0, 255)), (11, (255, 2, 0, 255)), (2 ** 32 - 1, (255, 2, 0, 255))]


def test_hand_made_values_through_the_colour_model():
    got = M.shade_distance([v for v, _ in HAND_DISTANCE])
    for (v, want), px in zip(HAND_DISTANCE, got):
        assert tuple(px.tolist()) == want, (v, px, want)
    got = M.shade_distance([v for v, _ in HAND_NO_LINE], line=0.0)
    for (v, want), px in zip(HAND_NO_LINE, got):
        assert tuple(px.tolist()) == want, (v, px, want)
    got = M.shade_count(np.array([v for v, _ in HAND_COUNT], np.uint32), 3, 10)
    for (v, want), px in zip(HAND_COUNT, got):
        assert tuple(px.tolist()) == want, (v, px, want)
    # lo == hi: v <= lo comes first
    assert M.shade_count(np.array([4, 5, 6], np.uint32), 5, 5)[:, :2].tolist() == [[0, 255], [0, 255], [255, 2]]
    # a huge range in 64 bits: (2^32 - 2) * 255 // (2^32 - 1) = 254
    assert M.shade_count(np.array([2 ** 32 - 2], np.uint32), 0, 2 ** 32 - 1)[0].tolist() == [255, 4, 0, 255]


# ------------------------------------------------------------------------------------------------- CPU: build invariants

@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_field_kernels_spill_nothing(extra):
    """Exactly twelve field_kernel<ACCEL, GEN>: no VGPR spill; no scratch for spheres and primitive lists (GEN 0 / 1); the
    expression-program interpreter's per-lane scratch (GEN 2 / 3) within the bound of the render and query kernels."""
    from test_build_invariants import HIPCC, assert_no_vgpr_spill, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void field_kernel<")}
    assert len(kernels) == 12, sorted(kernels)
    assert_no_vgpr_spill(kernels, 800)


def test_the_shade_field_kernel_uses_no_scratch():
    from test_build_invariants import HIPCC, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage((), "rm_frame_ops.hip")
    k = [r for n, r in usage.items() if n.startswith("shade_field_kernel(")]
    assert len(k) == 1, sorted(usage)
    assert k[0]["VGPRs Spill"] == 0 and k[0]["ScratchSize [bytes/lane]"] == 0, k[0]


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope="module")
def fctx(rm):
    """A context of its own.  Interpreter only: field_kernel is ahead-of-time, so is the entry it is compared with."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    return c


def load(rm, oracle, ctx, scene, accel):
    """Makes `scene` (a preset index or "mixed") under `accel` the context's active scene -> the rm.Scene."""
    sc = rm.Scene(accel, ctx=ctx)
    if scene == "mixed":
        sc.loadPrims(oracle.OracleScene(accel="None", prims=oracle.synthetic_mixed_prims(40)).prims())
    else:
        sc.loadPreset(scene)
    return sc


def oracle_scene(oracle, scene, accel):
    if scene == "mixed":
        return oracle.OracleScene(accel=accel, prims=oracle.synthetic_mixed_prims(40))
    return oracle.OracleScene(preset=scene, accel=accel)


_boxes = {}


def root_box(rm, oracle, scene):
    """(root_min, root_max) of the scene's BVH root box (rm_scene_get_info; a scene without a structure reports none), from a
    host-only context."""
    if scene not in _boxes:
        info = load(rm, oracle, rm.Context(None), scene, "BVH").info()
        _boxes[scene] = (np.array(info["root_min"], np.float64), np.array(info["root_max"], np.float64))
    return _boxes[scene]


def skew_lattice(rm, box, time=0.0):
    """19 x 13 x 3 points, no axis-aligned step, centred on the root box and 1.3 times its size along every index: partial
    8 x 8 tiles in both directions, more than one slice, a last workgroup that is not full."""
    mn, mx = box
    c, h = (mn + mx) / 2, (mx - mn) / 2
    s = 2.6 * h / np.array([18, 12, 2])
    du = np.array([s[0], 0.05 * s[1], 0.004 * s[2]])
    dv = np.array([0.04 * s[0], s[1], -0.006 * s[2]])
    dw = np.array([-0.05 * s[0], 0.03 * s[1], s[2]])
    return lattice(rm, c - (9 * du + 6 * dv + dw), du, dv, dw, (19, 13, 3), time)


def line_lattice(rm, box, through, shape, time=0.0):
    """n points in a row (along whichever index has them) on a diagonal of the root box, `through` (a point inside the box)
    at the middle index and 2.2 half-sizes of the box to either side of it: both ends lie outside along every axis."""
    mn, mx = box
    h = (mx - mn) / 2
    n = max(shape)
    m = (n - 1) // 2
    step = 2.2 * h / m
    zero = np.zeros(3)
    return lattice(rm, np.asarray(through, np.float64) - m * step, *[step if k == n else zero for k in shape], shape, time)


def field(rm, ctx, lat, dist=True, dist32=True, count=True):
    """rm_scene_field through ctypes, each requested output between two sentinel guards -> (dist, dist32, count), None for
    the ones not asked for."""
    N = rm._native
    n = lat.nu * lat.nv * lat.nw
    raws = [np.full(n * size + 2 * GUARD, FILL, np.uint8) if want else None for want, size in ((dist, 8), (dist32, 4), (count, 4))]
    N.check(ctx._h, N.lib().rm_scene_field(ctx._h, C.byref(lat), *[None if r is None else C.c_void_p(r.ctypes.data + GUARD) for r in raws]))
    out = []
    for raw, dt in zip(raws, (np.float64, np.float32, np.uint32)):
        if raw is None:
            out.append(None)
            continue
        assert (raw[:GUARD] == FILL).all() and (raw[len(raw) - GUARD:] == FILL).all(), "written outside the buffer"
        out.append(np.frombuffer(raw[GUARD:len(raw) - GUARD].tobytes(), dt))
    return out


def check_inputs(box, pts, dist, whole):
    """The lattice leaves the root box on every side (a line: at both ends, along every axis) and holds points inside an object."""
    mn, mx = box
    assert (dist < 0).any(), "no lattice point inside an object"
    for c in range(3):
        assert pts[:, c].min() < mn[c] and pts[:, c].max() > mx[c], (c, pts[:, c].min(), pts[:, c].max(), mn, mx)
    if whole:  # the outermost layer of every index lies outside
        p = pts.reshape(3, 13, 19, 3)
        outside = ((p < mn) | (p > mx)).any(axis=-1)
        assert outside[0].all() and outside[-1].all() and outside[:, 0].all() and outside[:, -1].all() and outside[:, :, 0].all() and outside[:, :, -1].all()


def inside_point(rm, ctx, box, time):
    """A point inside an object: the skewed lattice's point of the most negative distance."""
    lat = skew_lattice(rm, box, time)
    d, _, _ = field(rm, ctx, lat, dist32=False, count=False)
    assert d.min() < 0, "the skewed lattice has no point inside an object"
    return points_of(rm, lat)[np.argmin(d)].astype(np.float64)


SCENES = [(3, "None", 0.0), (3, "BVH", 0.0), (3, "Octree", 0.0), (12, "None", 0.7), (12, "BVH", 0.7), (5, "Octree", 0.0), (7, "Octree", 0.0),
          ("mixed", "BVH", 0.0)]
SHAPES = [(19, 13, 3), (1, 70, 1), (64, 1, 1)]


def make_lattice(rm, ctx, box, shape, time):
    if shape == (19, 13, 3):
        return skew_lattice(rm, box, time)
    return line_lattice(rm, box, inside_point(rm, ctx, box, time), shape, time)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("scene,accel,time", SCENES)
def test_the_field_is_the_distance_of_its_points(rm, oracle, fctx, scene, accel, time, shape):
    load(rm, oracle, fctx, scene, accel)
    box = root_box(rm, oracle, scene)
    lat = make_lattice(rm, fctx, box, shape, time)
    pts = points_of(rm, lat)
    dist, d32, cnt = field(rm, fctx, lat)
    assert fctx.last_kernel().startswith("field_kernel<"), fctx.last_kernel()
    check_inputs(box, pts.astype(np.float64), dist, shape == (19, 13, 3))
    fctx.scene_set_time(time)
    want_d, want_c = fctx.scene_distance(pts)
    assert same_bits(dist, want_d), (scene, accel, shape, int((dist != want_d).sum()))
    assert np.array_equal(cnt, want_c) and same_bits(d32, dist.astype(np.float32))
    assert cnt.max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene,accel,time", [(3, "None", 0.0), (3, "BVH", 0.0), (3, "Octree", 0.0), (12, "None", 0.7)])
def test_the_field_equals_the_oracle_alone(rm, oracle, fctx, scene, accel, time):
    load(rm, oracle, fctx, scene, accel)
    lat = skew_lattice(rm, root_box(rm, oracle, scene), time)
    dist, _, cnt = field(rm, fctx, lat, dist32=False)
    osc = oracle_scene(oracle, scene, accel)
    want = [osc.distance(p, time) for p in M.points(*vectors(lat))]
    assert len(want) == 741
    wd, wc = np.array([w[0] for w in want], np.float64), np.array([w[1] for w in want], np.uint32)
    assert (dist == wd).all() and same_bits(dist, wd) and np.array_equal(cnt, wc), (int((dist != wd).sum()), int((cnt != wc).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("scene,accel", [(3, "BVH"), (7, "Octree")])
def test_the_sqrt_length_build(rm, oracle, fctx, scene, accel):
    load(rm, oracle, fctx, scene, accel)
    fctx.set_option("length", 1)
    try:
        lat = skew_lattice(rm, root_box(rm, oracle, scene))
        dist, d32, cnt = field(rm, fctx, lat)
        assert fctx.last_kernel().startswith("field_kernel<") and fctx.last_kernel().endswith("[length=sqrt]")
        want_d, want_c = fctx.scene_distance(points_of(rm, lat))
        assert same_bits(dist, want_d) and np.array_equal(cnt, want_c) and same_bits(d32, dist.astype(np.float32))
    finally:
        fctx.set_option("length", 0)


@pytest.mark.gpu
def test_the_lattices_time_is_its_own(rm, oracle, fctx):
    load(rm, oracle, fctx, 12, "None")
    fctx.scene_set_time(0.2)
    lat = skew_lattice(rm, root_box(rm, oracle, 12), 0.7)
    pts = points_of(rm, lat)
    dist, _, cnt = field(rm, fctx, lat, dist32=False)
    osc = oracle_scene(oracle, 12, "None")
    want = [osc.distance(p, 0.7) for p in pts]
    assert same_bits(dist, np.array([w[0] for w in want], np.float64)) and np.array_equal(cnt, np.array([w[1] for w in want], np.uint32))
    after, _ = fctx.scene_distance(pts[:64])  # rm_scene_set_time's value was kept
    at02 = np.array([osc.distance(p, 0.2)[0] for p in pts[:64]], np.float64)
    assert same_bits(after, at02) and not same_bits(after, dist[:64])


@pytest.mark.gpu
def test_a_run_time_compiled_scene(rm, oracle, gpu_ctx):
    """A default context (specialise = 1): rm_scene_distance runs the scene's own compiled kernel, the field the ahead-of-time one."""
    assert gpu_ctx.get_option("specialise") == 1
    load(rm, oracle, gpu_ctx, 12, "BVH")
    lat = skew_lattice(rm, root_box(rm, oracle, 12), 0.7)
    dist, d32, cnt = field(rm, gpu_ctx, lat)
    assert gpu_ctx.last_kernel().startswith("field_kernel<")
    gpu_ctx.scene_set_time(0.7)
    want_d, want_c = gpu_ctx.scene_distance(points_of(rm, lat))
    assert same_bits(dist, want_d) and np.array_equal(cnt, want_c)


@pytest.mark.gpu
def test_absent_outputs_and_empty_lattices(rm, oracle, fctx):
    import torch
    N = rm._native
    load(rm, oracle, fctx, 3, "BVH")
    box = root_box(rm, oracle, 3)
    lat = skew_lattice(rm, box)
    full = field(rm, fctx, lat)
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        got = field(rm, fctx, lat, *[bool(m) for m in mask])
        for m, g, f in zip(mask, got, full):
            assert (g is None) if not m else same_bits(g, f), mask
    before = fctx.last_kernel()
    raw = np.full(4096, FILL, np.uint8)
    guard = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    for shape in ((0, 13, 3), (19, 0, 3), (19, 13, 0)):
        empty = skew_lattice(rm, box)
        empty.nu, empty.nv, empty.nw = shape
        assert N.lib().rm_scene_field(fctx._h, C.byref(empty), vp(raw), vp(raw[1024:]), vp(raw[2048:])) == N.RM_OK
        assert N.lib().rm_scene_field(fctx._h, C.byref(empty), None, None, None) == N.RM_OK
        assert N.lib().rm_scene_field_device(fctx._h, C.byref(empty), C.c_void_p(guard.data_ptr()), C.c_void_p(guard.data_ptr() + 1024),
                                             C.c_void_p(guard.data_ptr() + 2048), None) == N.RM_OK
    torch.cuda.synchronize()
    assert (raw == FILL).all() and (guard.cpu().numpy() == FILL).all() and fctx.last_kernel() == before
    d, c = fctx.field(*SKEW, shape=(0, 5, 2))
    assert d.shape == (2, 5, 0) and c.shape == (2, 5, 0)


@pytest.mark.gpu
def test_the_device_entry_equals_the_host_entry_on_two_streams(rm, oracle, fctx):
    import torch
    N = rm._native
    load(rm, oracle, fctx, 3, "Octree")
    box = root_box(rm, oracle, 3)
    lats = [skew_lattice(rm, box), line_lattice(rm, box, (box[0] + box[1]) / 2, (1, 70, 1))]
    want = [field(rm, fctx, lat) for lat in lats]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for st, lat in zip(streams, lats):  # both in flight before either is waited for
        n = lat.nu * lat.nv * lat.nw
        with torch.cuda.stream(st):
            bufs = [torch.full((n * size + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda") for size in (8, 4, 4)]
            N.check(fctx._h, N.lib().rm_scene_field_device(fctx._h, C.byref(lat), *[C.c_void_p(b.data_ptr() + GUARD) for b in bufs],
                                                           C.c_void_p(st.cuda_stream)))
            got.append(bufs)
    for st in streams:
        st.synchronize()
    for bufs, w in zip(got, want):
        for b, x in zip(bufs, w):
            raw = b.cpu().numpy()
            assert (raw[:GUARD] == FILL).all() and (raw[len(raw) - GUARD:] == FILL).all()
            assert raw[GUARD:len(raw) - GUARD].tobytes() == x.tobytes()
    # torch's default stream, one output alone
    n = 741
    only = torch.empty(n, dtype=torch.float32, device="cuda")
    N.check(fctx._h, N.lib().rm_scene_field_device(fctx._h, C.byref(lats[0]), None, C.c_void_p(only.data_ptr()), None, None))
    torch.cuda.synchronize()
    assert only.cpu().numpy().tobytes() == want[0][1].tobytes()


@pytest.mark.gpu
def test_the_host_path_across_a_chunk(rm, oracle, fctx):
    """2048 x 2049 points of one evaluation each (preset 0: one sphere): a chunk of the host path is 2048 whole rows =
    4 194 304 points, the last row goes alone."""
    load(rm, oracle, fctx, 0, "None")
    lat = lattice(rm, (-2.5, -2.5, 0.3), (5 / 2048, 1e-5, 0), (2e-5, 5 / 2049, 0), (0, 0, 0), (2048, 2049, 1))
    n = 2048 * 2049
    dist, d32, cnt = field(rm, fctx, lat)
    pts = points_of(rm, lat)
    want_d, want_c = fctx.scene_distance(pts)
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()  # noqa: E731
    assert digest(dist) == digest(want_d) and digest(cnt) == digest(want_c) and digest(d32) == digest(want_d.astype(np.float32))
    assert (cnt == 1).all() and (dist < 0).any() and (dist > 0).any()
    osc = oracle_scene(oracle, 0, "None")
    first = (1 << 22) // 2048 * 2048
    assert first == 1 << 22 and first + 2048 == n  # the last row is the one behind the 4 M boundary
    for i in (first - 2048, first - 1, first, n - 1):  # first and last point of the rows on both sides of it
        assert dist[i] == osc.distance(pts[i])[0], i


def hand_values():
    return np.array([v for v, _ in HAND_DISTANCE], np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_shade_field_for_both_maps(rm, oracle, fctx, n):
    import torch
    N = rm._native
    load(rm, oracle, fctx, 3, "Octree")
    d, c = fctx.field_slice("z", 0.0, 1.6, (64, 64))
    assert (d < 0).sum() >= 100 and (d > 0).sum() >= 100 and c.max() > c.min()
    order = np.argsort(np.abs(d.reshape(-1)), kind="stable")  # from the zero line outwards: both signs from the start
    dist = np.concatenate([hand_values(), d.reshape(-1)[order]])[:n]
    count = np.concatenate([[v for v, _ in HAND_COUNT], c.reshape(-1)[order]]).astype(np.uint32)[:n]

    def run(sh, values):
        raw = np.full(4 * n + 2 * GUARD, FILL, np.uint8)
        N.check(fctx._h, N.lib().rm_shade_field(fctx._h, C.byref(sh), n, vp(values), C.c_void_p(raw.ctypes.data + GUARD)))
        assert fctx.last_kernel() == "shade_field_kernel"
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + 4 * n:] == FILL).all(), "written outside the image"
        dev_v = torch.from_numpy(values.view(np.uint8)).cuda()
        dev = torch.full((4 * n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        N.check(fctx._h, N.lib().rm_shade_field_device(fctx._h, C.byref(sh), n, C.c_void_p(dev_v.data_ptr()), C.c_void_p(dev.data_ptr() + GUARD), None))
        torch.cuda.synchronize()
        assert dev.cpu().numpy().tobytes() == raw.tobytes(), "the device entry differs from the host entry"
        return raw[GUARD:GUARD + 4 * n].reshape(n, 4)

    for kw in (dict(), dict(line=0.0), dict(range=0.7, band=0.031, line=0.004)):
        got = run(shade_args(rm, **kw), dist)
        want = M.shade_distance(dist, kw.get("range", 2.0), kw.get("band", 0.25), kw.get("line", 0.02))
        assert np.array_equal(got, want), (kw, np.nonzero((got != want).any(axis=1))[0][:5])
    got = run(shade_args(rm), dist)
    for k, (_, px) in enumerate(HAND_DISTANCE[:n]):
        assert tuple(got[k].tolist()) == px, k
    hi = int(count.max())
    for lo_, hi_ in ((3, 10), (0, max(hi, 1)), (5, 5), (0, 2 ** 32 - 1)):
        got = run(shade_args(rm, map=1, lo=lo_, hi=hi_), count)
        assert np.array_equal(got, M.shade_count(count, lo_, hi_)), (lo_, hi_)
    five = np.array([4, 5, 6], np.uint32)[:n]  # lo == hi: v <= lo gives s = 0
    raw = np.zeros((len(five), 4), np.uint8)
    N.check(fctx._h, N.lib().rm_shade_field(fctx._h, C.byref(shade_args(rm, map=1, lo=5, hi=5)), len(five), vp(five), vp(raw)))
    assert raw.tolist() == [[0, 255, 0, 255], [0, 255, 0, 255], [255, 2, 0, 255]][:len(five)]
    # the Python method, numpy and torch
    assert np.array_equal(fctx.shade_field(dist), M.shade_distance(dist))
    assert np.array_equal(fctx.shade_field(torch.from_numpy(count.view(np.int32)).cuda(), map="count", lo=3, hi=10).cpu().numpy(),
                          M.shade_count(count, 3, 10))


@pytest.mark.gpu
def test_field_entries_leave_armed_diagnostics_alone(rm, oracle, fctx):
    import torch
    W, H = 64, 48
    sc = load(rm, oracle, fctx, 3, "BVH")
    sc.camera.setAngles(0.2, 0.5)
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    fctx._attach_diag(acc)
    d, c = fctx.field_slice("y", 0.1, 4.0, (48, 40))
    assert fctx.last_kernel().startswith("field_kernel<")
    dd, _ = fctx.field_slice("y", 0.1, 4.0, (48, 40), device=True)
    fctx.shade_field(d)
    assert fctx.last_kernel() == "shade_field_kernel"
    fctx.shade_field(dd)
    fctx.shade_field(c, map="count", hi=20)
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "a field entry fired the diagnostics"
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    torch.cuda.synchronize()
    got = fctx.decode_acc(acc)
    s = bufs[2].cpu().numpy().view(np.uint16).astype(np.int64)
    i = bufs[3].cpu().numpy().view(np.uint16).astype(np.int64)
    assert got == {"total_sdf": int(s.sum()), "total_iters": int(i.sum()), "max_sdf": int(s.max()), "min_sdf": int(s.min())}


@pytest.mark.gpu
def test_the_python_conveniences(rm, oracle, fctx):
    import torch
    sc = load(rm, oracle, fctx, 12, "BVH")
    origin, du, dv, shape = fctx.slice_lattice("x", 0.25, 3.0, (40, 24))
    assert shape == (40, 24) and origin.dtype == du.dtype == dv.dtype == np.float32
    assert origin.tolist() == [0.25, np.float32(-3 + 0.075), -2.875] and du.tolist() == [0, np.float32(0.15), 0] and dv.tolist() == [0, 0, 0.25]
    d, c = fctx.field_slice("x", 0.25, 3.0, (40, 24), time=0.7)
    fd, fc = fctx.field(origin, du, dv, shape=shape, time=0.7)
    assert d.shape == c.shape == (24, 40) and d.dtype == np.float64 and c.dtype == np.uint32 and same_bits(d, fd) and same_bits(c, fc)
    pts = fctx.lattice_points(origin, du, dv, shape=shape)
    assert pts.shape == (1, 24, 40, 3) and pts.dtype == np.float32 and (pts[..., 0] == 0.25).all()
    fctx.scene_set_time(0.7)
    want_d, want_c = fctx.scene_distance(pts)
    assert same_bits(d, want_d) and same_bits(c, want_c)
    # a volume, float32 distances, no counts
    v32, none = fctx.field(*SKEW, shape=(9, 5, 4), time=0.7, dist32=True, count=False)
    v64, vc = fctx.field(*SKEW, shape=(9, 5, 4), time=0.7)
    assert none is None and v32.shape == vc.shape == (4, 5, 9) and v32.dtype == np.float32 and same_bits(v32, v64.astype(np.float32))
    # the device forms
    td, tc = fctx.field(*SKEW, shape=(9, 5, 4), time=0.7, device=True)
    t32, _ = fctx.field(*SKEW, shape=(9, 5, 4), time=0.7, dist32=True, device=True)
    torch.cuda.synchronize()
    assert td.is_cuda and tc.is_cuda and td.dtype == torch.float64 and tc.dtype == torch.int32 and tuple(td.shape) == (4, 5, 9)
    assert same_bits(td.cpu().numpy(), v64) and same_bits(tc.cpu().numpy(), vc) and same_bits(t32.cpu().numpy(), v32)
    # Scene.distanceField uses the scene's own time
    sc.updateTime(0.7)
    sd, scnt = sc.distanceField(*SKEW, shape=(9, 5, 4))
    assert same_bits(sd, v64) and same_bits(scnt, vc)
    sc.updateTime(0.2)
    sd2, _ = sc.distanceField(*SKEW, shape=(9, 5, 4))
    assert not same_bits(sd2, v64) and same_bits(sd2, fctx.field(*SKEW, shape=(9, 5, 4), time=0.2)[0])
