"""The distance rule on the CPU (include/rm_raymarch.h, "distances"): the numpy restatement tests/edt_model.py against a
brute-force minimum over all pairs and against scipy.ndimage.distance_transform_edt where scipy is importable,
rm_lattice_cubic, the layout of rm_edt_info, the argument checks of the entries on a host-only context, and the Python helpers
of Edt on numpy inputs.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_model as E  # noqa: E402
import parts_model as P  # noqa: E402

NAN = float("nan")
OK, INVALID, UNSUPPORTED, NO_DEVICE = 0, -1, -2, -3
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
SKEWED = ((-2.0, -2.05, 2.0), (0.125, 0.004, -0.003), (-0.005, 0.125, 0.006), (0.004, -0.003, -0.125), (33, 33, 33))
DENSITIES = (0.2, 0.5, 0.9, 0.999)


def brute(s):
    """The minimum over all pairs, point by point."""
    s = np.asarray(s, bool)
    out = np.zeros(s.shape, np.int64)
    outside = np.argwhere(~s).astype(np.int64)
    for at in np.argwhere(s):
        out[tuple(at)] = ((outside - at) ** 2).sum(axis=1).min() if len(outside) else E.FAR
    return out.astype(np.int32)


@pytest.mark.parametrize("shape", [(5, 7, 9), (1, 7, 9), (5, 1, 9), (5, 7, 1), (1, 1, 6), (1, 1, 1), (2, 0, 3)])
def test_the_model_equals_the_minimum_over_all_pairs(shape):
    rng = np.random.default_rng(sum(shape))
    for density in DENSITIES + (0.0, 1.0):
        s = rng.random(shape) < density
        got = E.edt(s)
        assert got.dtype == np.int32 and got.shape == s.shape
        assert np.array_equal(got, brute(s)), (shape, density)
        assert ((got > 0) == s).all()
        info = E.info(s, got)
        assert (info["n_points"], info["n_set"]) == (s.size, int(s.sum()))
        if s.all() and s.size:
            assert (got == E.FAR).all() and (info["max_d2"], info["argmax"]) == (E.FAR, 0)
        if not s.any():
            assert (info["max_d2"], info["argmax"]) == (0, -1)


@pytest.mark.parametrize("shape", [(21, 10, 67), (3, 5, 130), (2, 3, 256), (9, 9, 1), (1, 1, 1)])  # [nw, nv, nu] of the issue's shapes
def test_the_model_equals_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(shape[2])
    for density in DENSITIES:
        s = rng.random(shape) < density
        if s.all():
            s.reshape(-1)[s.size // 2] = False  # scipy has no rule for a volume without background
        assert np.array_equal(np.sqrt(E.edt(s).astype(np.float64)), ndimage.distance_transform_edt(s)), (shape, density)


def test_the_argmax_is_the_smallest_index_and_the_helpers_follow_the_rule():
    s = np.zeros((5, 5, 11), bool)
    s[1:4, 1:4, 1:4] = True
    s[1:4, 1:4, 6:9] = True     # two cubes of 27: the centres tie at d2 = 4
    s[2, 2, 4:6] = True         # a bridge one point thick
    d2 = E.edt(s)
    info = E.info(s, d2)
    assert (info["max_d2"], info["argmax"]) == (4, 2 + 11 * (2 + 5 * 2)) and d2[2, 2, 7] == 4
    labels = P.label(s)
    assert labels.max() == 0 and E.max_by_part(d2, labels).tolist() == [4]
    # eroding by 3 leaves the two centres; the opening restores what lies closer than sqrt(3) to them: the cubes less their
    # corners, and not the bridge
    cut = E.eroded(s, d2, 3) < 0
    assert cut.sum() == 2 and P.label(cut).max() == 1 and E.max_by_part(d2, P.label(cut)).tolist() == [4, 4]
    back = E.opened(s, 3) < 0
    assert (back <= s).all() and not back[2, 2, 4:6].any() and back[2, 2, 2] and back[2, 2, 1] and back[1, 1, 2] and not back[1, 1, 1]
    assert back.sum() == 2 * (27 - 8)
    assert not (E.opened(s, 100) < 0).any() and np.array_equal(E.opened(s, 1) < 0, s)


# ------------------------------------------------------------------------------------------------- the library without a device

@pytest.fixture(scope="module")
def bare(rm):
    c = rm.Context(None)
    yield c
    c.close()


def lattice(rm, shape):
    return rm.make_lattice(*UNIT, shape=shape)


def cubic(rm, lat):
    step = C.c_double(-7.0)
    rc = rm._native.lib().rm_lattice_cubic(C.byref(lat), C.byref(step))
    return rc, step.value


def test_lattice_cubic(rm):
    assert cubic(rm, lattice(rm, (4, 5, 6))) == (OK, 1.0)
    eighth = rm.make_lattice((-2, -2, -2), (0.125, 0, 0), (0, 0.125, 0), (0, 0, 0.125), shape=(33, 33, 33))
    assert cubic(rm, eighth) == (OK, 0.125)
    # the same lattice turned by rm_make_transform's rotation, its steps rounded to binary32
    m = rm.make_transform(0.0, 0.0, 0.0, (0.3, 0.4, 0.5)).reshape(4, 4)[:3, :3].astype(np.float64)
    assert np.allclose(m @ m.T, np.eye(3), atol=1e-6) and abs(m[0, 1]) > 0.05
    steps = [(0.125 * m[a]).astype(np.float32) for a in range(3)]
    turned = rm.make_lattice((-2, -2, -2), *steps, shape=(33, 33, 33))
    rc, step = cubic(rm, turned)
    x, y, z = (float(c) for c in steps[0])
    assert rc == OK and step == np.sqrt((x * x + y * y) + z * z) and abs(step - 0.125) < 1e-7
    assert rm.lattice_cubic(turned) == step
    # not cubic: skewed steps, unequal steps; *step is left alone
    assert cubic(rm, rm.make_lattice(*SKEWED[:4], shape=SKEWED[4])) == (UNSUPPORTED, -7.0)
    assert rm.lattice_cubic(rm.make_lattice(*SKEWED[:4], shape=SKEWED[4])) is None
    unequal = ((0, 0, 0), (0.125, 0, 0), (0, 0.125, 0), (0, 0, 0.25))
    assert cubic(rm, rm.make_lattice(*unequal, shape=(9, 9, 9))) == (UNSUPPORTED, -7.0)
    # an axis of one point does not take part; the first axis that does gives the step; none: 1.0
    assert cubic(rm, rm.make_lattice(*unequal, shape=(9, 9, 1))) == (OK, 0.125)
    assert cubic(rm, rm.make_lattice(*unequal, shape=(1, 1, 9))) == (OK, 0.25)
    assert cubic(rm, rm.make_lattice(*unequal, shape=(1, 9, 9))) == (UNSUPPORTED, -7.0)
    assert cubic(rm, rm.make_lattice(*SKEWED[:4], shape=(1, 1, 1))) == (OK, 1.0)
    assert cubic(rm, rm.make_lattice(*unequal, shape=(0, 9, 9)))[0] == UNSUPPORTED  # counts of 0 do not take part either
    # the tolerance: a relative 5e-6 passes, 2e-5 does not
    near = ((0, 0, 0), (1, 0, 0), (0, 1 + 5e-6, 0), (0, 0, 1))
    far = ((0, 0, 0), (1, 0, 0), (0, 1 + 2e-5, 0), (0, 0, 1))
    tilted = ((0, 0, 0), (1, 0, 0), (2e-5, 1, 0), (0, 0, 1))
    assert cubic(rm, rm.make_lattice(*near, shape=(3, 3, 3))) == (OK, 1.0)
    assert cubic(rm, rm.make_lattice(*far, shape=(3, 3, 3)))[0] == UNSUPPORTED
    assert cubic(rm, rm.make_lattice(*tilted, shape=(3, 3, 3)))[0] == UNSUPPORTED
    # null arguments and a malformed lattice
    L = rm._native.lib()
    bad = lattice(rm, (3, 3, 3))
    bad.reserved = 1
    step = C.c_double(0.0)
    assert L.rm_lattice_cubic(None, C.byref(step)) == INVALID and L.rm_lattice_cubic(C.byref(bad), C.byref(step)) == INVALID
    assert L.rm_lattice_cubic(C.byref(eighth), None) == INVALID


def test_the_info_is_32_bytes_and_the_names_are_exported(rm):
    N = rm._native
    assert C.sizeof(N.rm_edt_info) == 32 and [f[0] for f in N.rm_edt_info._fields_] == ["n_points", "n_set", "max_d2", "argmax"]
    assert N.RM_EDT_FAR == 2 ** 31 - 1 == E.FAR
    for name in ("rm_edt_field_device", "rm_scene_edt", "rm_lattice_cubic"):
        assert getattr(N.lib(), name) is not None and name in N.SIGNATURES
    assert rm.Edt is rm.context.Edt and hasattr(rm.Scene, "edt")
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(rm.Context.edt_field) == ["self", "values", "origin", "du", "dv", "dw", "shape", "iso", "side", "device"]
    assert params(rm.Context.edt) == ["self", "origin", "du", "dv", "dw", "shape", "iso", "time", "side", "device", "exact"]
    assert params(rm.Context.open_field) == ["self", "values", "origin", "du", "dv", "dw", "shape", "r2", "iso", "device"]
    assert params(rm.Context.edt_box)[1:3] == ["cells", "margin"] and "side" in params(rm.Scene.edt)


def test_the_argument_checks_come_ahead_of_the_range_and_the_device(rm, bare):
    N = rm._native
    L = N.lib()
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += (-base) % 256

    def at(offset):
        return C.c_void_p(base + offset)

    p = at(0)
    good = lattice(rm, (17, 17, 17))
    bad = lattice(rm, (17, 17, 17))
    bad.reserved = 1
    big = lattice(rm, (1025, 1024, 1024))
    longest, too_long, too_wide = lattice(rm, (46341, 1, 1)), lattice(rm, (46342, 1, 1)), lattice(rm, (40000, 26000, 1))
    assert 46340 ** 2 <= 2 ** 31 - 2 < 46341 ** 2 and 39999 ** 2 + 25999 ** 2 > 2 ** 31 - 2 and 40000 * 26000 <= 2 ** 30
    # the square of 2^30 points is inside the limit by the rule itself: 2 * 32767^2 = 2^31 - 2^17 + 2
    square = lattice(rm, (32768, 32768, 1))
    assert 2 * 32767 ** 2 <= 2 ** 31 - 2 and 32768 * 32768 == 2 ** 30
    host = "host-only context: there is no CPU distance transform"

    def msg():
        return L.rm_last_error(bare._h).decode()

    def edt(lat=good, values=p, vt=0, iso=0.0, side=0, d2=p, info=p):
        return L.rm_edt_field_device(bare._h, C.byref(lat) if lat is not None else None, values, vt, iso, side, d2, info, None), msg()

    assert L.rm_edt_field_device(None, C.byref(good), p, 0, 0.0, 0, p, p, None) == INVALID
    assert edt(lat=None)[0] == INVALID and edt(lat=bad) == (INVALID, "rm_lattice.reserved must be 0")
    assert edt(lat=big)[0] == INVALID and "more than 2^30 lattice points" in edt(lat=big)[1]
    assert edt(values=None) == (INVALID, "null values")
    assert edt(iso=NAN) == (INVALID, "non-finite iso") and edt(iso=float("inf"))[0] == INVALID
    for side in (-1, 2):
        assert edt(side=side) == (INVALID, "side must be RM_PARTS_INSIDE or RM_PARTS_OUTSIDE")
    assert edt(vt=2) == (INVALID, "value_type must be RM_MESH_F64 or RM_MESH_F32")
    assert edt(values=at(4)) == (INVALID, "values must be aligned to their type") and edt(values=at(2), vt=1)[0] == INVALID
    assert edt(d2=None) == (INVALID, "null d2") and edt(info=None) == (INVALID, "null info")
    assert edt(d2=at(2)) == (INVALID, "d2 must be 4-byte aligned")
    assert edt(info=at(4)) == (INVALID, "info must be 8-byte aligned")
    assert edt() == (NO_DEVICE, host) and edt(side=1, vt=1, values=at(4), d2=at(4)) == (NO_DEVICE, host)
    # the range refusal: behind the argument checks, ahead of the device
    assert edt(lat=longest) == (NO_DEVICE, host) and edt(lat=square) == (NO_DEVICE, host)
    for lat in (too_long, too_wide):
        rc, text = edt(lat=lat)
        assert rc == UNSUPPORTED and "INT32_MAX - 1" in text
        assert edt(lat=lat, side=2)[0] == INVALID and edt(lat=lat, info=None)[0] == INVALID
    # counts of 1 and of 0 are fine; without a point neither values nor d2 are asked for
    assert edt(lat=lattice(rm, (17, 1, 1))) == (NO_DEVICE, host)
    assert edt(lat=lattice(rm, (5, 0, 3)), values=None, d2=None) == (NO_DEVICE, host)
    assert edt(lat=lattice(rm, (5, 0, 3)), values=None, d2=None, info=None) == (INVALID, "null info")

    info = N.rm_edt_info()

    def scene(lat=good, iso=0.0, side=0, inf=info):
        return L.rm_scene_edt(bare._h, C.byref(lat) if lat is not None else None, iso, side, None, C.byref(inf) if inf is not None else None), msg()

    assert L.rm_scene_edt(None, C.byref(good), 0.0, 0, None, C.byref(info)) == INVALID
    assert scene(lat=None)[0] == INVALID and scene(lat=bad) == (INVALID, "rm_lattice.reserved must be 0")
    assert scene(lat=big)[0] == INVALID
    assert scene(iso=NAN) == (INVALID, "non-finite iso") and scene(side=2)[0] == INVALID
    assert scene(inf=None) == (INVALID, "null info")
    assert scene(lat=too_long)[0] == UNSUPPORTED and scene(lat=too_long, side=2)[0] == INVALID
    assert scene() == (NO_DEVICE, host)
    # the Python entries say the same without a device, and refuse an unknown side themselves
    with pytest.raises(N.RmError) as e:
        bare.edt_field(np.zeros(8), *UNIT, (2, 2, 2))
    assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        bare.edt_field(np.zeros(8), *UNIT, (2, 2, 2), side="both")


# ------------------------------------------------------------------------------------------------- Edt on numpy inputs

def make_edt(rm, s, side="inside", step=1.0):
    d2 = E.edt(s)
    info = E.info(s, d2)
    return rm.Edt(d2, info["n_points"], info["n_set"], info["max_d2"], info["argmax"], side, step), d2


def test_edt_distance_erosion_and_maxima_by_part(rm):
    s = np.zeros((5, 5, 11), bool)
    s[1:4, 1:4, 1:4] = True
    s[1:4, 1:4, 6:9] = True
    s[2, 2, 4:6] = True
    edt, d2 = make_edt(rm, s, step=0.125)
    assert edt.at == (2, 2, 2) and edt.max_d2 == 4 and edt.inradius == 0.25 and edt.n_set == int(s.sum())
    dist = edt.distance()
    assert dist.dtype == np.float64 and np.array_equal(dist, np.sqrt(d2.astype(np.float64)) * 0.125)
    for r2 in (0, 1, 2, 4, 5):
        got = edt.eroded(r2)
        assert got.dtype == np.float64 and np.array_equal(got, E.eroded(s, d2, r2)), r2
    parts = rm.Parts(P.label(E.eroded(s, d2, 2) < 0), s.size, 0, 2, [])
    got = edt.max_by_part(parts)
    assert got.dtype == np.int64 and got.tolist() == E.max_by_part(d2, parts.labels).tolist() == [4, 4]
    # the whole lattice in the set: FAR is an infinite distance
    full, _ = make_edt(rm, np.ones((2, 3, 4), bool))
    assert full.max_d2 == E.FAR and full.at == (0, 0, 0) and np.isinf(full.distance()).all() and full.inradius == float("inf")
    empty, _ = make_edt(rm, np.zeros((2, 3, 4), bool))
    assert empty.argmax == -1 and empty.at is None and empty.inradius == 0.0
    # no step, no world distance
    skew, _ = make_edt(rm, s, step=None)
    with pytest.raises(ValueError):
        skew.distance()
    with pytest.raises(ValueError):
        skew.inradius
