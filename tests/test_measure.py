"""Measures (include/rm_raymarch.h, "measures") without a GPU: the numpy model against a brute-force loop, the sparse rule
against the dense one on analytic 1-Lipschitz fields, rm_measure_world (host-only) against the model bit for bit, and the
argument checks of every entry on a host-only context."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import measure_model as M
import mesh_sparse_model as S

NAN = float("nan")


# ------------------------------------------------------------------------------------------------- the model by brute force

def brute(values, nu, nv, nw, iso):
    v = [float(x) for x in np.asarray(values, np.float64).reshape(-1)]

    def at(i, j, k):
        return v[(k * nv + j) * nu + i]

    def inside(i, j, k):
        return at(i, j, k) < iso  # NaN: False

    n_inside = n_nonfinite = 0
    sum1, sum2, crossings = [0, 0, 0], [0] * 6, [0, 0, 0]
    lo, hi = [M.INT32_MAX] * 3, [-1] * 3
    for k in range(nw):
        for j in range(nv):
            for i in range(nu):
                x = at(i, j, k)
                if x != x or x in (float("inf"), float("-inf")):
                    n_nonfinite += 1
                p = (i, j, k)
                for A, n in enumerate((nu, nv, nw)):
                    q = list(p)
                    q[A] += 1
                    if q[A] < n and inside(*q) != inside(*p):
                        crossings[A] += 1
                if not inside(*p):
                    continue
                n_inside += 1
                for c in range(3):
                    sum1[c] += p[c]
                    lo[c], hi[c] = min(lo[c], p[c]), max(hi[c], p[c])
                for e, (a, b) in enumerate(M.PAIRS):
                    sum2[e] += p[a] * p[b]
    return dict(n_points=nu * nv * nw, n_inside=n_inside, n_nonfinite=n_nonfinite, sum1=tuple(sum1), sum2=tuple(sum2), crossings=tuple(crossings),
                lo=tuple(lo), hi=tuple(hi), n_blocks=0, n_kept=0, n_blocks_inside=0)


@pytest.mark.parametrize("shape", [(5, 4, 3), (9, 9, 9)])
def test_the_dense_model_against_a_loop(shape):
    rng = np.random.default_rng(sum(shape))
    v = rng.standard_normal(shape[0] * shape[1] * shape[2])
    v[::7] = 0.25  # equality with iso is outside
    v[3], v[11], v[20] = NAN, float("inf"), float("-inf")
    got = M.measure_dense(v, *shape, 0.25)
    assert got == brute(v, *shape, 0.25)
    assert 0 < got["n_inside"] < got["n_points"] and got["n_nonfinite"] == 3 and min(got["crossings"]) > 0
    none = M.measure_dense(np.full(v.shape, 1.0), *shape, 0.0)
    assert none == brute(np.full(v.shape, 1.0), *shape, 0.0) and none["lo"] == (M.INT32_MAX,) * 3 and none["hi"] == (-1, -1, -1)
    # a slice: no edges along the missing axis, and its cross-section is n_inside
    flat = M.measure_dense(v[:shape[0] * shape[1]], shape[0], shape[1], 1, 0.25)
    assert flat == brute(v[:shape[0] * shape[1]], shape[0], shape[1], 1, 0.25) and flat["crossings"][2] == 0 and flat["hi"][2] <= 0


# ------------------------------------------------------------------------------------------------- sparse == dense

def union_of_spheres(points, spheres):
    """min over (centre, radius) of |x - c| - r at float32 points [..., 3], in binary64: 1-Lipschitz."""
    p = np.asarray(points, np.float32).astype(np.float64)
    d = np.full(p.shape[:-1], np.inf)
    for c, r in spheres:
        d = np.minimum(d, np.sqrt(((p - np.asarray(c, np.float64)) ** 2).sum(-1)) - r)
    return d


def sparse_case(vecs, shape, spheres, iso):
    """(dense record, sparse record, slot, dist) of a union of spheres over a lattice, the coarse decision by mesh_sparse_model."""
    nu, nv, nw = shape
    k, j, i = np.meshgrid(np.arange(nw), np.arange(nv), np.arange(nu), indexing="ij")
    values = union_of_spheres(S._points(*vecs, i, j, k), spheres)
    dist = union_of_spheres(S.centres(*vecs, *shape), spheres)
    slot, lst = S.blocks(dist, iso, S.bound(*vecs, *shape, 1.0))
    tiles = S.tiles(values, *shape, lst)
    return M.measure_dense(values, *shape, iso), M.measure_sparse(tiles, slot, lst, dist, *shape, iso), slot, dist


def cube(origin, step):
    return ((origin,) * 3, (step, 0, 0), (0, step, 0), (0, 0, step))


TWO = [((0.3, -0.2, 0.1), 0.9), ((-0.8, 0.6, -0.5), 0.55)]
SPARSE_CASES = {
    "9^3: one block, the last point its own": (cube(-1.5, 0.375), (9, 9, 9), TWO, 0.0),
    "10^3: two blocks, the second with one cell": (cube(-1.5, 0.33), (10, 10, 10), TWO, 0.0),
    "17^3: two blocks, the last point the last block's": (cube(-2.0, 0.25), (17, 17, 17), TWO, 0.0),
    "18^3: three blocks": (cube(-2.0, 0.25), (18, 18, 18), TWO, 0.0),
    "25x13x20": (((-2.0, -1.5, -1.75), (0.17, 0.01, 0), (0, 0.25, 0), (0.02, 0, 0.19)), (25, 13, 20), TWO, 0.0),
    "17^3, iso 0.15": (cube(-2.0, 0.25), (17, 17, 17), TWO, 0.15),
    "17^3, iso -0.2": (cube(-2.0, 0.25), (17, 17, 17), TWO, -0.2),
}


@pytest.mark.parametrize("name", sorted(SPARSE_CASES))
def test_the_sparse_rule_equals_the_dense_one(name):
    vecs, shape, spheres, iso = SPARSE_CASES[name]
    dense, sparse, slot, _ = sparse_case(vecs, shape, spheres, iso)
    assert M.same_measure(dense, sparse), (dense, sparse)
    assert 0 < dense["n_inside"] < dense["n_points"] and min(dense["crossings"]) > 0
    assert sparse["n_blocks"] == len(slot) == int(np.prod(S.lattice_blocks(*shape))) and sparse["n_kept"] == int((slot >= 0).sum())


def test_dropped_blocks_inside_and_outside_take_the_closed_forms():
    """33^3 over [-4, 4]^3, blocks 2 wide, bound 3: a sphere of radius 4.8 about the corner (-4, -4, -4) leaves the corner
    block dropped as inside and the far blocks dropped as outside; a sphere of radius 0.6 leaves most blocks dropped as outside."""
    vecs, shape = cube(-4.0, 0.25), (33, 33, 33)
    dense, sparse, slot, dist = sparse_case(vecs, shape, [((-4.0, -4.0, -4.0), 4.8)], 0.0)
    dropped = slot < 0
    n_in, n_out = int((dropped & (dist < 0)).sum()), int((dropped & ~(dist < 0)).sum())
    assert n_in > 0 and n_out > 0 and sparse["n_blocks_inside"] == n_in and sparse["n_kept"] == 64 - n_in - n_out
    assert M.same_measure(dense, sparse), (dense, sparse)
    dense, sparse, slot, dist = sparse_case(vecs, shape, [((0.4, -0.3, 0.2), 0.6)], 0.0)
    assert M.same_measure(dense, sparse) and sparse["n_blocks_inside"] == 0 and 0 < sparse["n_kept"] < 32 and dense["n_inside"] > 0
    # a large sphere in the middle: the eight central blocks lie inside
    dense, sparse, slot, dist = sparse_case(vecs, shape, [((0.0, 0.0, 0.0), 4.8)], 0.0)
    assert M.same_measure(dense, sparse) and sparse["n_blocks_inside"] == 8


# ------------------------------------------------------------------------------------------------- the library, host only

@pytest.fixture(scope="module")
def bare(rm):
    c = rm.Context(None)
    yield c
    c.close()


def lattice(rm, vecs, shape, time=0.0):
    return rm.make_lattice(*vecs, shape=shape, time=time)


def record_of(rm, d):
    r = rm._native.rm_measure()
    for f in M.FIELDS:
        if isinstance(d[f], tuple):
            getattr(r, f)[:] = d[f]
        else:
            setattr(r, f, d[f])
    return r


def bits(x):
    return struct.pack("<d", x)


def test_the_records_have_their_sizes_and_the_entries_their_signatures(rm):
    N = rm._native
    assert C.sizeof(N.rm_measure) == 176 and N.rm_measure.lo.offset == 120 and N.rm_measure.n_blocks.offset == 144 and N.rm_measure.reserved.offset == 168
    assert C.sizeof(N.rm_measure_world) == 120
    for name, n_args in (("rm_measure_field_device", 7), ("rm_measure_tiles_device", 10), ("rm_scene_measure", 6), ("rm_measure_world", 3)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == n_args and hasattr(N.lib(), name), name


SKEWED = ((0.5, -1.25, 2.0), (0.25, 0.03125, 0.0), (0.0625, -0.1875, 0.015625), (0.0, 0.125, 0.3125))  # det < 0: left-handed


def test_measure_world_equals_the_model_bit_for_bit(rm):
    u, v, w = (np.array(x, np.float64) for x in SKEWED[1:])
    assert np.dot(u, np.cross(v, w)) < 0
    rng = np.random.default_rng(5)
    full = M.measure_dense(rng.standard_normal(9 * 7 * 5), 9, 7, 5, 0.1)
    empty = M.measure_dense(np.ones(9 * 7 * 5), 9, 7, 5, 0.0)
    assert full["n_inside"] > 0 and empty["n_inside"] == 0
    for rec in (full, empty):
        lat = lattice(rm, SKEWED, (9, 7, 5))
        got = rm.measure_world(lat, record_of(rm, rec))
        want = M.world(SKEWED, rec)
        for f in ("cell_volume", "volume", "area_estimate"):
            assert bits(getattr(got, f)) == bits(want[f]), f
        for f in ("centroid", "second", "projected_area"):
            assert [bits(x) for x in getattr(got, f)] == [bits(x) for x in want[f]], f
    assert all(x != x for x in got.centroid) and got.volume == 0.0 and got.second == (0.0,) * 6  # the empty record
    # by hand: a 2 x 2 x 2 block of inside points on a unit lattice at the origin is a cube of side 2 about (0.5, 0.5, 0.5)
    eight = M.measure_dense(np.full(8, -1.0), 2, 2, 2, 0.0)
    unit = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
    got = rm.measure_world(lattice(rm, unit, (2, 2, 2)), record_of(rm, eight))
    assert got.volume == 8.0 and got.centroid == (0.5, 0.5, 0.5) and got.projected_area == (0.0, 0.0, 0.0)
    assert np.allclose(got.second, (8.0 * 4 / 12,) * 3 + (0.0,) * 3, rtol=1e-15)  # V s^2 / 12 per axis
    # null arguments and a lattice the field entries refuse
    L = rm._native.lib()
    lat, rec, out = lattice(rm, unit, (2, 2, 2)), record_of(rm, eight), rm._native.rm_measure_world()
    assert L.rm_measure_world(None, C.byref(rec), C.byref(out)) == -1 and L.rm_measure_world(C.byref(lat), None, C.byref(out)) == -1
    assert L.rm_measure_world(C.byref(lat), C.byref(rec), None) == -1
    lat.reserved = 1
    assert L.rm_measure_world(C.byref(lat), C.byref(rec), C.byref(out)) == -1


def test_measure_world_against_a_direct_sum_over_the_inside_points(rm):
    """Independent of the order of operations the header fixes: every inside point stands for the parallelepiped of its cell,
    centred on it.  Volume N |det|; centroid the mean of the points; second moments the sum over the points of
    (x - c)(x - c)^T |det| plus each cell's own (u u^T + v v^T + w w^T) |det| / 12; the projected area along index axis A the
    crossings times |step_B x step_C|.  On the skewed left-handed lattice the off-diagonal terms are all non-zero, so a mixed-up
    index would show.  Tolerance: some 300 binary64 sums of terms of like size, 1e-12 relative to the largest entry."""
    nu, nv, nw = 9, 7, 5
    rng = np.random.default_rng(11)
    values = rng.standard_normal(nu * nv * nw)
    rec = M.measure_dense(values, nu, nv, nw, 0.1)
    o, u, v, w = (np.asarray(x, np.float32).astype(np.float64) for x in SKEWED)
    k, j, i = np.nonzero(values.reshape(nw, nv, nu) < 0.1)
    x = o + i[:, None] * u + j[:, None] * v + k[:, None] * w
    cv = abs(np.linalg.det(np.stack([u, v, w])))
    c = x.mean(axis=0)
    second = cv * (x - c).T @ (x - c) + len(x) * cv / 12.0 * (np.outer(u, u) + np.outer(v, v) + np.outer(w, w))
    got = rm.measure_world(lattice(rm, SKEWED, (nu, nv, nw)), record_of(rm, rec))
    assert len(x) == rec["n_inside"] > 50
    assert np.isclose(got.cell_volume, cv, rtol=1e-13) and np.isclose(got.volume, len(x) * cv, rtol=1e-13)
    assert np.allclose(got.centroid, c, rtol=0, atol=1e-13 * np.abs(x).max())
    want = [second[p, q] for p, q in M.PAIRS]
    assert np.allclose(got.second, want, rtol=0, atol=1e-12 * np.abs(second).max()) and min(abs(s) for s in want[3:]) > 1e-6 * np.abs(second).max()
    steps = (u, v, w)
    area = [rec["crossings"][A] * np.linalg.norm(np.cross(steps[(A + 1) % 3], steps[(A + 2) % 3])) for A in range(3)]
    assert np.allclose(got.projected_area, area, rtol=1e-13) and np.isclose(got.area_estimate, 2.0 / 3.0 * sum(area), rtol=1e-13)
    inertia = rm.context.measure_from_record(lattice(rm, SKEWED, (nu, nv, nw)), record_of(rm, rec)).inertia()
    assert np.allclose(inertia, np.trace(second) * np.eye(3) - second, rtol=0, atol=1e-12 * np.abs(second).max())


INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -3
HOST = "host-only context: there is no CPU measure"
OVERFLOW = "the sums of this lattice do not fit 64 bits: n_points * (max count - 1)^2 reaches 2^63"
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))


def test_the_argument_checks_in_their_order(rm, bare):
    N = rm._native
    L = N.lib()
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += (-base) % 256

    def at(offset):
        return C.c_void_p(base + offset)

    p = at(0)
    good = lattice(rm, UNIT, (17, 17, 17))
    bad = lattice(rm, UNIT, (17, 17, 17))
    bad.reserved = 1

    def msg():
        return L.rm_last_error(bare._h).decode()

    # ---- rm_measure_field_device: the lattice, 2^30 points, null values, null measure, iso, value_type, alignment; the device
    def field(lat=good, values=p, vt=0, iso=0.0, measure=p):
        return L.rm_measure_field_device(bare._h, C.byref(lat) if lat is not None else None, values, vt, iso, measure, None), msg()

    assert L.rm_measure_field_device(None, C.byref(good), p, 0, 0.0, p, None) == INVALID
    assert field(lat=None)[0] == INVALID and field(lat=bad, values=None) == (INVALID, "rm_lattice.reserved must be 0")
    big = lattice(rm, UNIT, (1025, 1024, 1024))
    assert field(lat=big, values=None) == (INVALID, "more than 2^30 lattice points: the measure does not split a volume")
    assert field(values=None, measure=None) == (INVALID, "null values")
    assert field(measure=None, iso=NAN) == (INVALID, "null measure")
    assert field(iso=float("inf"), vt=2) == (INVALID, "non-finite iso")
    assert field(vt=2, values=at(4)) == (INVALID, "value_type must be RM_MESH_F64 or RM_MESH_F32")
    assert field(values=at(4)) == (INVALID, "values must be aligned to their type")
    assert field(values=at(4), vt=1, measure=at(4)) == (INVALID, "measure must be 8-byte aligned")
    assert field(values=at(2), vt=1) == (INVALID, "values must be aligned to their type")
    assert field() == (NO_DEVICE, HOST) and field(values=at(4), vt=1) == (NO_DEVICE, HOST)
    # counts of 1 and of 0 are fine; without a point no values are asked for
    assert field(lat=lattice(rm, UNIT, (17, 17, 1))) == (NO_DEVICE, HOST)
    assert field(lat=lattice(rm, UNIT, (17, 0, 3)), values=None) == (NO_DEVICE, HOST)

    # ---- rm_measure_tiles_device: the lattice, a count below 2, n_kept, the nulls, iso, alignment, the overflow; the device
    def tiles(lat=good, slot=p, lst=p, k=2, dist=p, tl=p, iso=0.0, measure=p):
        return L.rm_measure_tiles_device(bare._h, C.byref(lat) if lat is not None else None, slot, lst, k, dist, tl, iso, measure, None), msg()

    below = "every lattice count must be at least 2: a slice goes through rm_measure_field_device"
    assert L.rm_measure_tiles_device(None, C.byref(good), p, p, 2, p, p, 0.0, p, None) == INVALID
    assert tiles(lat=None)[0] == INVALID and tiles(lat=bad, k=-1) == (INVALID, "rm_lattice.reserved must be 0")
    assert tiles(lat=lattice(rm, UNIT, (65535, 65535, 2)), k=-1) == (INVALID, "more than 2^24 blocks")
    for shape in ((17, 17, 1), (1, 17, 17), (17, 0, 17)):
        assert tiles(lat=lattice(rm, UNIT, shape), k=-1) == (INVALID, below)
    assert tiles(k=-1, measure=None) == (INVALID, "n_kept must be in [0, n_blocks]") and tiles(k=9)[1] == "n_kept must be in [0, n_blocks]"
    assert tiles(measure=None, slot=None) == (INVALID, "null measure")
    assert tiles(slot=None, dist=None) == (INVALID, "null slot")
    assert tiles(dist=None, lst=None) == (INVALID, "null dist")
    assert tiles(lst=None, iso=NAN) == (INVALID, "null list or tiles") and tiles(tl=None)[1] == "null list or tiles"
    assert tiles(iso=NAN, slot=at(2)) == (INVALID, "non-finite iso")
    assert tiles(slot=at(2), dist=at(4)) == (INVALID, "slot and list must be 4-byte aligned") and tiles(lst=at(6))[1] == "slot and list must be 4-byte aligned"
    for kw in (dict(dist=at(4)), dict(tl=at(12)), dict(measure=at(20))):
        assert tiles(**kw) == (INVALID, "dist, tiles and measure must be 8-byte aligned"), kw
    assert tiles() == (NO_DEVICE, HOST) and tiles(k=8) == (NO_DEVICE, HOST)
    assert tiles(k=0, lst=None, tl=None) == (NO_DEVICE, HOST)  # nothing kept: no list, no tiles
    # 65535 x 1025 x 129 points in 2^24 blocks: n_points * 65534^2 is beyond 2^63 -- refused ahead of the device, behind the arguments
    huge = lattice(rm, UNIT, (65535, 1025, 129))
    assert 65535 * 1025 * 129 * 65534 ** 2 >= 2 ** 63
    assert tiles(lat=huge) == (UNSUPPORTED, OVERFLOW) and tiles(lat=huge, measure=None) == (INVALID, "null measure")
    fits = lattice(rm, UNIT, (4097, 2049, 1025))  # 2^24 blocks, 2^33 points, 2^24 per squared index: below 2^63
    assert 4097 * 2049 * 1025 * 4096 ** 2 < 2 ** 63 and tiles(lat=fits) == (NO_DEVICE, HOST)

    # ---- rm_scene_measure: its own arguments, the overflow, the device
    out, info = N.rm_measure(), N.rm_sparse_info()

    def scene(lat=good, iso=0.0, lipschitz=1.0, o=out):
        return L.rm_scene_measure(bare._h, C.byref(lat) if lat is not None else None, iso, lipschitz, C.byref(o) if o is not None else None,
                                  C.byref(info)), msg()

    assert L.rm_scene_measure(None, C.byref(good), 0.0, 1.0, C.byref(out), None) == INVALID
    assert scene(lat=None)[0] == INVALID and scene(lat=bad, o=None) == (INVALID, "rm_lattice.reserved must be 0")
    assert scene(lat=lattice(rm, UNIT, (17, 17, 1)), o=None) == (INVALID, below)
    assert scene(o=None, iso=NAN) == (INVALID, "null measure")
    assert scene(iso=NAN, lipschitz=0.0) == (INVALID, "non-finite iso")
    assert scene(lipschitz=0.0) == (INVALID, "lipschitz must be finite and > 0") and scene(lipschitz=NAN)[0] == INVALID
    assert scene(lat=huge) == (UNSUPPORTED, OVERFLOW)
    assert scene() == (NO_DEVICE, HOST)
    # the Python entries say the same without a device
    with pytest.raises(N.RmError) as e:
        bare.measure_field(np.zeros(8), *UNIT, (2, 2, 2))
    assert e.value.code == NO_DEVICE


# ------------------------------------------------------------------------------------------------- build invariants

def test_the_measure_kernels_spill_nothing():
    import shutil
    from test_build_invariants import HIPCC, resource_usage
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage((), "rm_measure.hip")
    names = ("void measure_field_kernel<double>", "void measure_field_kernel<float>", "measure_tiles_kernel", "measure_blocks_kernel", "measure_final_kernel")
    kernels = {n: r for n, r in usage.items() if n.split("(")[0] in names}
    assert len(kernels) == 5, sorted(usage)
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "rm_measure.hip" in open(os.path.join(root, "cpu_raymarcher_amd", "csrc", "Makefile")).read()
