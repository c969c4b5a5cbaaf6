"""The parts rule on the CPU (include/rm_raymarch.h, "parts"): the numpy restatement tests/parts_model.py against
scipy.ndimage.label where scipy is importable and on hand-made cases where it is not, the sum-of-records property against
tests/measure_model.py, the layout of rm_parts_info, the argument checks of the three entries on a host-only context, and the
Python helpers of Parts on numpy inputs.  Nothing here needs a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_model as M  # noqa: E402
import parts_model as P  # noqa: E402

NAN = float("nan")
INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -3
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))


def brute_label(s):
    """Flood fill in index order: the first unlabelled point of S starts the next part."""
    s = np.asarray(s, bool)
    nw, nv, nu = s.shape
    out = np.full(s.shape, -1, np.int32)
    count = 0
    for k, j, i in zip(*np.nonzero(s)):
        if out[k, j, i] >= 0:
            continue
        stack = [(k, j, i)]
        out[k, j, i] = count
        while stack:
            c, b, a = stack.pop()
            for z, y, x in ((c, b, a - 1), (c, b, a + 1), (c, b - 1, a), (c, b + 1, a), (c - 1, b, a), (c + 1, b, a)):
                if 0 <= z < nw and 0 <= y < nv and 0 <= x < nu and s[z, y, x] and out[z, y, x] < 0:
                    out[z, y, x] = count
                    stack.append((z, y, x))
        count += 1
    return out


def hand_made():
    cases = {}
    two = np.zeros((6, 7, 9), bool)
    two[1:3, 1:4, 1:4] = True
    two[3:5, 4:6, 5:8] = True
    cases["two boxes"] = (two, 2)
    u = np.zeros((1, 6, 7), bool)  # a U whose smallest index is the tip of its second arm
    u[0, 1:5, 1] = True
    u[0, 4, 1:6] = True
    u[0, 0:5, 5] = True
    cases["U"] = (u, 1)
    k, j, i = np.indices((5, 6, 7))
    cases["checkerboard"] = ((i + j + k) % 2 == 0, (5 * 6 * 7 + 1) // 2)
    cases["empty"] = (np.zeros((3, 4, 5), bool), 0)
    cases["full"] = (np.ones((3, 4, 5), bool), 1)
    return cases


@pytest.mark.parametrize("name", sorted(hand_made()))
def test_the_model_on_hand_made_cases(name):
    s, n_parts = hand_made()[name]
    got = P.label(s)
    assert got.dtype == np.int32 and got.shape == s.shape
    assert np.array_equal(got, brute_label(s)), name
    assert P.info(s, got) == dict(n_points=s.size, n_set=int(s.sum()), n_parts=n_parts, gave_up=0)
    assert ((got >= 0) == s).all()
    if name == "U":
        assert got[0, 0, 5] == 0 and int(np.argmax(s.reshape(-1))) == 5  # the part's number comes from a dead-end tip
    if name == "checkerboard":
        assert np.array_equal(got[s], np.arange(n_parts))


@pytest.mark.parametrize("density", [0.2, 0.31, 0.5, 0.9])
def test_the_model_equals_the_flood_fill_on_random_volumes(density):
    rng = np.random.default_rng(int(density * 100))
    s = rng.random((9, 12, 19)) < density
    assert np.array_equal(P.label(s), brute_label(s))


@pytest.mark.parametrize("density", [0.2, 0.31, 0.5, 0.9])
def test_the_model_equals_scipy_on_random_volumes(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 100))
    for shape in ((9, 12, 19), (21, 10, 67)):
        volume = rng.random(shape) < density
        assert np.array_equal(P.label(volume), ndimage.label(volume)[0].astype(np.int32) - 1)


@pytest.mark.parametrize("density", [0.2, 0.31, 0.5, 0.9])
def test_the_records_add_up_to_the_measure_of_the_whole(density):
    rng = np.random.default_rng(5)
    nu, nv, nw = 19, 12, 9
    v = rng.random(nu * nv * nw) - density
    v[::11] = 0.0
    v[3], v[40] = NAN, float("-inf")
    s = P.in_set(v, nu, nv, nw, 0.0)
    labels = P.label(s)
    n_parts = P.info(s, labels)["n_parts"]
    records = P.part_records(labels, n_parts + 2)
    whole = M.measure_dense(v, nu, nv, nw, 0.0)
    total = P.sum_records(records)
    assert total == {f: whole[f] for f in P.SHARED}
    assert all(r["n_inside"] > 0 and r["n_points"] == nu * nv * nw and r["n_nonfinite"] == 0 for r in records[:n_parts])
    for r in records[n_parts:]:  # the empty record
        assert r["n_inside"] == 0 and r["lo"] == (M.INT32_MAX,) * 3 and r["hi"] == (-1,) * 3 and r["crossings"] == (0, 0, 0)
    # a record is the brute-force sum over its part, crossings by the rule: edges with one end in S, for the end in S
    p = n_parts // 2
    k, j, i = (x.astype(np.int64) for x in np.nonzero(labels == p))
    assert records[p]["n_inside"] == len(i) and records[p]["sum1"] == (int(i.sum()), int(j.sum()), int(k.sum()))
    assert records[p]["sum2"][3:] == (int((i * j).sum()), int((j * k).sum()), int((k * i).sum()))
    cross = [0, 0, 0]
    for z, y, x in zip(k, j, i):
        for c, (dz, dy, dx) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
            for sign in (-1, 1):
                zz, yy, xx = z + sign * dz, y + sign * dy, x + sign * dx
                if 0 <= zz < nw and 0 <= yy < nv and 0 <= xx < nu and not s[zz, yy, xx]:
                    cross[c] += 1
    assert records[p]["crossings"] == tuple(cross)
    # the outside: the complement, NaN and equality included; its records sum to the same crossings
    outside = P.in_set(v, nu, nv, nw, 0.0, side=1)
    assert (outside != s).all() and outside.reshape(-1)[3] and outside.reshape(-1)[0]
    out_labels = P.label(outside)
    assert P.sum_records(P.part_records(out_labels, int(out_labels.max()) + 1))["crossings"] == whole["crossings"]
    # fewer records than parts: the first ones, unchanged
    assert P.part_records(labels, 2) == records[:2]


# ------------------------------------------------------------------------------------------------- the library without a device

@pytest.fixture(scope="module")
def bare(rm):
    c = rm.Context(None)
    yield c
    c.close()


def lattice(rm, shape):
    return rm.make_lattice(*UNIT, shape=shape)


def test_the_info_is_32_bytes_and_the_names_are_exported(rm):
    N = rm._native
    assert C.sizeof(N.rm_parts_info) == 32 and [f[0] for f in N.rm_parts_info._fields_] == ["n_points", "n_set", "n_parts", "gave_up"]
    assert (N.RM_PARTS_INSIDE, N.RM_PARTS_OUTSIDE) == (0, 1)
    assert rm.Parts is rm.context.Parts and hasattr(rm.Scene, "parts") and hasattr(rm.Context, "parts_box")


def test_the_argument_checks_come_ahead_of_the_device(rm, bare):
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
    too_many = "more than 2^30 lattice points: the labelling does not split a volume"

    def msg():
        return L.rm_last_error(bare._h).decode()

    # ---- rm_label_field_device
    def label(lat=good, values=p, vt=0, iso=0.0, side=0, labels=p, info=p):
        return L.rm_label_field_device(bare._h, C.byref(lat) if lat is not None else None, values, vt, iso, side, labels, info, None), msg()

    host = "host-only context: there is no CPU labelling"
    assert L.rm_label_field_device(None, C.byref(good), p, 0, 0.0, 0, p, p, None) == INVALID
    assert label(lat=None)[0] == INVALID and label(lat=bad) == (INVALID, "rm_lattice.reserved must be 0")
    assert label(lat=big) == (INVALID, too_many)
    assert label(values=None) == (INVALID, "null values")
    assert label(iso=NAN) == (INVALID, "non-finite iso") and label(iso=float("inf"))[0] == INVALID
    for side in (-1, 2):
        assert label(side=side) == (INVALID, "side must be RM_PARTS_INSIDE or RM_PARTS_OUTSIDE")
    assert label(vt=2) == (INVALID, "value_type must be RM_MESH_F64 or RM_MESH_F32")
    assert label(values=at(4)) == (INVALID, "values must be aligned to their type") and label(values=at(2), vt=1)[0] == INVALID
    assert label(labels=None) == (INVALID, "null labels") and label(info=None) == (INVALID, "null info")
    assert label(labels=at(2)) == (INVALID, "labels must be 4-byte aligned")
    assert label(info=at(4)) == (INVALID, "info must be 8-byte aligned")
    assert label() == (NO_DEVICE, host) and label(side=1, vt=1, values=at(4), labels=at(4)) == (NO_DEVICE, host)
    # counts of 1 and of 0 are fine; without a point neither values nor labels are asked for
    assert label(lat=lattice(rm, (17, 1, 1))) == (NO_DEVICE, host)
    assert label(lat=lattice(rm, (5, 0, 3)), values=None, labels=None) == (NO_DEVICE, host)
    assert label(lat=lattice(rm, (5, 0, 3)), values=None, labels=None, info=None) == (INVALID, "null info")

    # ---- rm_measure_labels_device
    def measure(lat=good, labels=p, k=4, records=p):
        return L.rm_measure_labels_device(bare._h, C.byref(lat) if lat is not None else None, labels, k, records, None), msg()

    count = "n_records must be in [0, 2^20]"
    assert L.rm_measure_labels_device(None, C.byref(good), p, 4, p, None) == INVALID
    assert measure(lat=None)[0] == INVALID and measure(lat=bad) == (INVALID, "rm_lattice.reserved must be 0")
    assert measure(lat=big) == (INVALID, too_many)
    assert measure(labels=None) == (INVALID, "null labels")
    assert measure(k=-1) == (INVALID, count) and measure(k=2 ** 20 + 1) == (INVALID, count)
    assert measure(records=None) == (INVALID, "null records with n_records above 0")
    assert measure(labels=at(2)) == (INVALID, "labels must be 4-byte aligned")
    assert measure(records=at(4)) == (INVALID, "records must be 8-byte aligned")
    assert measure() == (NO_DEVICE, "host-only context: there is no CPU measure")
    assert measure(k=2 ** 20)[0] == NO_DEVICE and measure(k=0, records=None)[0] == NO_DEVICE
    # (a lattice of at most 2^30 points always fits the overflow rule: 2^30 * 65534^2 < 2^63, so that refusal is the scene
    # entry's and the measures' to show)
    assert 2 ** 30 * 65534 ** 2 < 2 ** 63

    # ---- rm_scene_parts
    out, info = (N.rm_measure * 4)(), N.rm_parts_info()

    def scene(lat=good, iso=0.0, side=0, k=4, records=out, inf=info):
        return L.rm_scene_parts(bare._h, C.byref(lat) if lat is not None else None, iso, side, None, k, records,
                                C.byref(inf) if inf is not None else None), msg()

    assert L.rm_scene_parts(None, C.byref(good), 0.0, 0, None, 4, out, C.byref(info)) == INVALID
    assert scene(lat=None)[0] == INVALID and scene(lat=bad) == (INVALID, "rm_lattice.reserved must be 0")
    assert scene(lat=big) == (INVALID, too_many)
    assert scene(iso=NAN) == (INVALID, "non-finite iso") and scene(side=2)[0] == INVALID
    assert scene(k=-1) == (INVALID, count) and scene(records=None) == (INVALID, "null records with n_records above 0")
    assert scene(inf=None) == (INVALID, "null info")
    assert scene() == (NO_DEVICE, host) and scene(k=0, records=None) == (NO_DEVICE, host)
    # the Python entries say the same without a device, and refuse an unknown side themselves
    with pytest.raises(N.RmError) as e:
        bare.label_field(np.zeros(8), *UNIT, (2, 2, 2))
    assert e.value.code == NO_DEVICE
    with pytest.raises(ValueError):
        bare.label_field(np.zeros(8), *UNIT, (2, 2, 2), side="both")


# ------------------------------------------------------------------------------------------------- Parts on numpy inputs

def make_parts(rm, labels, side="inside", iso=0.0):
    """A Parts as Context.label_field builds it, from the model's labels and records."""
    nw, nv, nu = labels.shape
    lat = lattice(rm, (nu, nv, nw))
    n_parts = int(labels.max()) + 1
    measures = []
    for d in P.part_records(labels, n_parts):
        r = rm._native.rm_measure()
        for f in M.FIELDS:
            if isinstance(d[f], tuple):
                getattr(r, f)[:] = d[f]
            else:
                setattr(r, f, d[f])
        measures.append(rm.context.measure_from_record(lat, r))
    return rm.Parts(labels, labels.size, int((labels >= 0).sum()), n_parts, measures, iso, side)


def test_parts_by_size_border_and_select(rm):
    s = np.zeros((8, 8, 9), bool)
    s[0:2, 0:2, 0:2] = True   # part 0: 8 points, at the border
    s[3:6, 3:6, 3:7] = True   # part 1: 36 points, inside
    s[6, 1, 1:3] = True       # part 2: 2 points, inside
    s[7, 7, 7:9] = True       # part 3: 2 points, at the far border (a tie with part 2)
    labels = P.label(s)
    parts = make_parts(rm, labels, iso=0.25)
    assert (parts.n_points, parts.n_set, parts.n_parts) == (s.size, int(s.sum()), 4) and len(parts.measures) == 4
    assert parts.by_size() == [1, 0, 2, 3]
    assert [parts.touches_border(p) for p in range(4)] == [True, False, False, True]
    assert parts.measures[1].world.volume == 36.0 and parts.measures[1].inertia().shape == (3, 3)
    # select mirrors the parts that are not kept about iso, in the values' own type, and nothing else
    rng = np.random.default_rng(2)
    for dtype in (np.float64, np.float32):
        v = np.where(s, 0.25 - rng.random(s.shape) - 0.01, 0.25 + rng.random(s.shape)).astype(dtype)
        v[0, 5, 5] = 0.25  # equal to iso: outside, and not touched
        got = parts.select(v, [1])
        assert got.dtype == dtype and got.shape == v.shape and got is not v
        dropped = s & (labels != 1)
        assert np.array_equal(got[~dropped], v[~dropped])
        assert np.array_equal(got[dropped], (dtype(2) * dtype(0.25) - v[dropped]).astype(dtype)) and (got[dropped] > 0.25).all()
        assert np.array_equal(P.in_set(got, 9, 8, 8, 0.25), labels == 1)
        assert np.array_equal(parts.select(v.reshape(-1), [0, 1, 2, 3]), v.reshape(-1))
        assert not P.in_set(parts.select(v, []), 9, 8, 8, 0.25).any()
    # on the outside a value equal to iso is in the set; mirrored it stays iso
    out_labels = P.label(~s)
    outer = make_parts(rm, out_labels, side="outside", iso=0.25)
    assert outer.n_parts == 1 and outer.touches_border(0)
    v = np.where(s, 0.0, 0.5)
    v[0, 5, 5] = 0.25
    got = outer.select(v, [])
    assert got[0, 5, 5] == 0.25 and np.array_equal(got[~s & (v != 0.25)], np.full(int((~s).sum()) - 1, 0.0))
