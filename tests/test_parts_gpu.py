"""Parts on the GPU (rm_label_field_device, rm_measure_labels_device, rm_scene_parts, Context.label_field / parts, Parts;
include/rm_raymarch.h, "parts").  Labels, info and records are integers with one right answer: they must equal
tests/parts_model.py's of the same values, exactly.  Every result read here has gave_up == 0 -- the Python entries raise
otherwise, and the raw entries' info is asserted.  No test provokes a fault or a hang."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import measure_model as M  # noqa: E402
import parts_model as P  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, OCTREE, BVH = 0, 1, 2
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
SKEWED = ((-2.0, -2.05, 2.0), (0.125, 0.004, -0.003), (-0.005, 0.125, 0.006), (0.004, -0.003, -0.125), (33, 33, 33))
SIDES = ("inside", "outside")


def spheres40():
    rng = np.random.default_rng(40)
    return rng.uniform(-1.5, 1.5, (40, 3)).astype(np.float32), rng.uniform(0.05, 0.25, 40)


def box(lo, hi, shape):
    """An axis-aligned lattice of `shape` points over [lo, hi]^3 (a count of 1: the plane at lo)."""
    step = [(hi - lo) / (n - 1) if n > 1 else 1.0 for n in shape]
    return ((lo, lo, lo), (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), shape)


@pytest.fixture(scope="module")
def pctx(rm):
    """A context of its own.  Interpreter only, like the measure tests': every launch here is ahead-of-time."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    yield c
    c.close()


def as_dict(m):
    return dict(m._asdict())


def assert_parts(parts, values, shape, iso, side, records):
    """Labels, info and the first `records` records are the model's of `values`."""
    nu, nv, nw = shape
    s = P.in_set(values, nu, nv, nw, iso, SIDES.index(side))
    want = P.label(s)
    labels = parts.labels if isinstance(parts.labels, np.ndarray) else parts.labels.cpu().numpy()
    assert labels.dtype == np.int32 and labels.shape == (nw, nv, nu)
    assert np.array_equal(labels, want), (shape, side)
    info = P.info(s, want)
    assert (parts.n_points, parts.n_set, parts.n_parts) == (info["n_points"], info["n_set"], info["n_parts"]), (shape, side)
    model = P.part_records(want, min(records, info["n_parts"]))
    assert [as_dict(m) for m in parts.measures] == model, (shape, side)
    return want, model


def random_values(rng, n, density, dtype):
    """Values about iso = 0.25 of which `density` lie below; some equal iso, one NaN, both infinities."""
    v = rng.random(n) - density + 0.25
    if n >= 16:
        v[::7] = 0.25
        v[3], v[5], v[9] = float("nan"), float("inf"), float("-inf")
    return v.astype(dtype)


# (67, 10, 21): a row longer than a wave and no multiple of 64 -- runs cut at lane 0, rows that end inside a wave --; rows of
# one, two and four waves and one point more; planes and lines; a single point; no point
SHAPES = [(67, 10, 21), (130, 5, 3), (64, 4, 4), (65, 4, 4), (256, 3, 2), (1, 1, 1), (1, 9, 9), (9, 1, 9), (9, 9, 1), (5, 0, 3)]


@pytest.mark.parametrize("shape", SHAPES)
def test_random_volumes_equal_the_model(rm, pctx, shape):
    nu, nv, nw = shape
    n = nu * nv * nw
    rng = np.random.default_rng(nu + 7 * nv)
    for density in (0.2, 0.31, 0.5, 0.9, 1.0, 0.0):  # 1.0: all in (but the planted values), 0.0: all out
        for dtype in (np.float64, np.float32):
            v = random_values(rng, n, density, dtype)
            if density in (1.0, 0.0):
                v = np.full(n, 0.0 if density else 1.0, dtype)
            for side in SIDES:
                parts = pctx.label_field(v, *UNIT, shape, iso=0.25, side=side, records=None)
                want, _ = assert_parts(parts, v, shape, 0.25, side, 1 << 20)
                assert len(parts.measures) == parts.n_parts
                if n:
                    assert pctx.last_kernel() == ("parts_measure_kernel" if parts.n_parts else "parts_relabel_kernel")
    assert n == 0 or parts.n_parts == 1  # all out, seen from the outside, came last: one part


def serpentine(nu, nv, nw):
    """One path that folds through the whole lattice (nv, nw odd): in every second plane every second row is full and the rows
    between them are walls with one door, at alternating ends; the planes between are walls with one door, at alternating
    corners.  Cut any door and the part falls in two."""
    s = np.zeros((nw, nv, nu), bool)
    s[::2, ::2, :] = True
    for k in range(0, nw, 2):
        for j in range(1, nv, 2):
            s[k, j, (nu - 1) if (j // 2) % 2 == 0 else 0] = True
    for k in range(1, nw, 2):
        s[(k, 0, 0) if (k // 2) % 2 else (k, nv - 1, nu - 1)] = True
    return s


def combs(nu, nv, nw):
    """Two combs whose teeth interleave along i -- one hangs from the row j = 0, the other stands on the row j = nv - 1, in every
    plane but the last -- and that meet only through a bridge in the last plane."""
    s = np.zeros((nw, nv, nu), bool)
    s[:-1, 0, :] = True
    s[:-1, :-2, 0::4] = True     # teeth down from j = 0
    s[:-1, -1, :] = True
    s[:-1, 2:, 2::4] = True      # teeth up from j = nv - 1
    s[-1, :, nu - 1] = True      # the bridge: the first comb's row end to the second's
    return s


def tip(nu, nv, nw):
    """A part whose smallest index is a dead-end tip: a hook that hangs down from a bar far along k."""
    s = np.zeros((nw, nv, nu), bool)
    s[0, 0, nu // 2] = True
    s[:, 0, nu // 2] = True
    s[-1, :, nu // 2] = True
    s[-1, -1, :] = True
    s[2:, -1, 0] = True
    return s


STRESS = {"serpentine": (serpentine, (33, 33, 9)), "combs": (combs, (33, 33, 9)), "tip": (tip, (33, 9, 17))}


@pytest.mark.parametrize("name", sorted(STRESS))
def test_long_chains_come_out_as_one_part(rm, pctx, name):
    make, shape = STRESS[name]
    s = make(*shape)
    v = np.where(s, -1.0, 1.0)
    parts = pctx.label_field(v, *UNIT, shape, records=4)
    assert_parts(parts, v, shape, 0.0, "inside", 4)
    assert parts.n_parts == 1 and parts.measures[0].n_inside == int(s.sum())


def test_the_checkerboard_numbers_every_point(rm, pctx):
    """65^3: 137 313 parts over 1 073 workgroups -- the scan takes a second step of RM_MESH_SCAN_STEP = 1024 -- and every
    workgroup numbers roots; the expected labels are a running count."""
    import torch
    n = 65
    k, j, i = np.indices((n, n, n))
    s = (i + j + k) % 2 == 0
    v = torch.from_numpy(np.where(s, -1.0, 1.0)).cuda()
    parts = pctx.label_field(v, *UNIT, (n, n, n), records=100, device=True)
    labels = parts.labels.cpu().numpy()
    want = np.full(s.shape, -1, np.int32)
    want[s] = np.arange(int(s.sum()), dtype=np.int32)
    assert np.array_equal(labels, want)
    assert (parts.n_points, parts.n_set, parts.n_parts) == (n ** 3, 137313, 137313) and (n ** 3 + 255) // 256 == 1073
    # a point of its own: no neighbour in the set, so every lattice edge at it crosses
    l = np.flatnonzero(s.reshape(-1))[:100]
    for p, m in enumerate(parts.measures):
        at = (int(l[p] % n), int(l[p] // n % n), int(l[p] // (n * n)))
        edges = tuple((1 if c > 0 else 0) + (1 if c < n - 1 else 0) for c in at)
        assert (m.n_inside, m.sum1, m.lo, m.hi, m.crossings) == (1, at, at, at, edges)


def test_a_shell_has_one_part_and_encloses_a_void(rm, pctx):
    x = np.linspace(-2.0, 2.0, 33)
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    v = np.abs(np.sqrt(xx * xx + y * y + z * z) - 1.0) - 0.2
    geom = box(-2.0, 2.0, (33, 33, 33))
    inside = pctx.label_field(v, *geom, side="inside")
    assert_parts(inside, v, geom[4], 0.0, "inside", 64)
    assert inside.n_parts == 1 and not inside.touches_border(0)
    outside = pctx.label_field(v, *geom, side="outside")
    assert_parts(outside, v, geom[4], 0.0, "outside", 64)
    assert outside.n_parts == 2 and [outside.touches_border(p) for p in range(2)] == [True, False]
    assert outside.by_size() == [0, 1] and outside.n_set + inside.n_set == 33 ** 3
    # the void is centred: its centroid is the origin up to the rounding of the lattice's binary32 step
    assert np.allclose(outside.measures[1].world.centroid, 0.0, atol=1e-6)


def load(ctx, scene, accel):
    if scene == "sphere":
        ctx.scene_from_preset(0, accel)  # one sphere of radius 1.5 about the origin
    else:
        ctx.scene_from_spheres(*spheres40(), accel)


@pytest.mark.parametrize("accel", [BVH, OCTREE])
def test_one_sphere_is_one_part_with_the_measure_of_the_whole(rm, pctx, accel):
    load(pctx, "sphere", accel)
    geom = box(-2.0, 2.0, (33, 33, 33))
    parts = pctx.parts(*geom)
    whole = pctx.measure(*geom, sparse=False)
    assert parts.n_parts == 1 and parts.n_set == whole.n_inside
    assert {f: as_dict(parts.measures[0])[f] for f in P.SHARED} == {f: as_dict(whole)[f] for f in P.SHARED}
    assert parts.measures[0].world.volume == whole.world.volume
    sc = rm.Scene("BVH", ctx=pctx)  # the exact field does not depend on the structure
    sc.loadPreset(0)
    again = sc.parts(*geom)
    assert np.array_equal(again.labels, parts.labels) and again.measures == parts.measures
    boxed = sc.parts(cells=(20, 20, 20))
    assert boxed.n_parts == 1 and boxed.n_points == 21 ** 3 and boxed.labels.shape == (21, 21, 21)
    assert pctx.get_option("exact") == 0


def scene_parts(rm, ctx, geom, iso, side, n_records, want_labels=True):
    """rm_scene_parts through ctypes, every output filled with 0xA5 bytes first."""
    N = rm._native
    lat = rm.make_lattice(*geom)
    n = lat.nu * lat.nv * lat.nw
    labels = np.full(n, -1515870811, np.int32)
    records = (N.rm_measure * max(n_records, 1))()
    info = N.rm_parts_info()
    C.memset(records, 0xA5, C.sizeof(records))
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    N.check(ctx._h, N.lib().rm_scene_parts(ctx._h, C.byref(lat), float(iso), SIDES.index(side), labels.ctypes.data_as(C.c_void_p) if want_labels else None,
                                           n_records, records if n_records else None, C.byref(info)))
    return labels.reshape(lat.nw, lat.nv, lat.nu), [rm.context.measure_from_record(lat, r) for r in records[:n_records]], info


@pytest.mark.parametrize("accel", [BVH, OCTREE])
def test_forty_spheres_equal_the_model_and_the_host_entry(rm, pctx, accel):
    """Option exact is 0 throughout: under the octree the scene's own field is the marchers' bound, so equality with
    Context.parts(exact=True) shows that the host entry samples the exact field whatever the option says."""
    load(pctx, "spheres40", accel)
    for geom in (box(-2.0, 2.0, (33, 33, 33)), SKEWED):
        for side in SIDES:
            vol, _ = pctx.field(*geom, count=False, device=True, exact=True)
            parts = pctx.parts(*geom, iso=0.05, side=side, records=64, exact=True)
            assert_parts(parts, vol.cpu().numpy(), geom[4], 0.05, side, 64)
            assert parts.n_parts > 1 or side == "outside"
            labels, measures, info = scene_parts(rm, pctx, geom, 0.05, side, 64)
            assert info.gave_up == 0 and (info.n_points, info.n_set, info.n_parts) == (parts.n_points, parts.n_set, parts.n_parts)
            assert np.array_equal(labels, parts.labels)
            assert measures[:parts.n_parts] == parts.measures[:64]
            for m in measures[parts.n_parts:]:
                assert m.n_inside == 0 and m.lo == (M.INT32_MAX,) * 3 and m.hi == (-1, -1, -1) and m.n_points == parts.n_points
            assert pctx.last_kernel() == "parts_measure_kernel"
    # no labels asked for, no records asked for
    _, _, info = scene_parts(rm, pctx, SKEWED, 0.05, "outside", 0, want_labels=False)  # (`parts`: the last of the loop)
    assert (info.n_points, info.n_set, info.n_parts, info.gave_up) == (33 ** 3, parts.n_set, parts.n_parts, 0)
    assert pctx.get_option("exact") == 0
    # without a scene the entry says so, behind its argument checks
    with rm.Context(0) as empty:
        N = rm._native
        lat = rm.make_lattice(*SKEWED)
        out, inf = (N.rm_measure * 2)(), N.rm_parts_info()
        assert N.lib().rm_scene_parts(empty._h, C.byref(lat), 0.0, 0, None, 2, out, C.byref(inf)) == -5
        assert N.lib().rm_scene_parts(empty._h, C.byref(lat), 0.0, 3, None, 2, out, C.byref(inf)) == -1


@pytest.fixture(scope="module")
def crumbs():
    """(67, 10, 21) at density 0.31 about iso 0.25, the model's labels and all its records: computed once, left unchanged."""
    shape = (67, 10, 21)
    v = random_values(np.random.default_rng(31), 67 * 10 * 21, 0.31, np.float64)
    want = P.label(P.in_set(v, *shape, 0.25))
    return shape, v, want, P.part_records(want, int(want.max()) + 1)


def raw_records(rm, ctx, lat, labels, n_records, guard=3):
    """rm_measure_labels_device into a buffer of n_records + guard records filled with a pattern -> int64 [n_records + guard, 22]."""
    import torch
    N = rm._native
    out = torch.full(((n_records + guard) * 22,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    N.check(ctx._h, N.lib().rm_measure_labels_device(ctx._h, C.byref(lat), C.c_void_p(labels.data_ptr()), n_records, C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out.cpu().numpy().reshape(-1, 22)


def test_fewer_and_more_records_than_parts(rm, pctx, crumbs):
    shape, v, want, model = crumbs
    n_parts = len(model)
    assert n_parts > 70
    lat = rm.make_lattice(*UNIT, shape=shape)
    few = pctx.label_field(v, *UNIT, shape, iso=0.25, records=5, device=True)
    assert few.n_parts == n_parts and [as_dict(m) for m in few.measures] == model[:5]
    # the raw entry: nothing behind the last record asked for is written
    raw = raw_records(rm, pctx, lat, few.labels, 5)
    assert (raw[5:] == 0x5A5A5A5A5A5A5A5A).all()
    got = [rm.context.measure_from_record(lat, rm._native.rm_measure.from_buffer_copy(raw[p].tobytes())) for p in range(5)]
    assert [as_dict(m) for m in got] == model[:5]
    # more records than parts: the empty record behind the parts, and again nothing behind the buffer
    raw = raw_records(rm, pctx, lat, few.labels, n_parts + 4)
    assert (raw[n_parts + 4:] == 0x5A5A5A5A5A5A5A5A).all()
    empty = rm._native.rm_measure.from_buffer_copy(raw[n_parts + 3].tobytes())
    assert (empty.n_points, empty.n_inside, tuple(empty.lo), tuple(empty.hi)) == (67 * 10 * 21, 0, (M.INT32_MAX,) * 3, (-1,) * 3)
    assert not raw[n_parts:n_parts + 4, 1:15].any() and not raw[n_parts:n_parts + 4, 18:].any()
    many = pctx.label_field(v, *UNIT, shape, iso=0.25, records=n_parts + 4)
    assert len(many.measures) == n_parts and [as_dict(m) for m in many.measures] == model
    # the records add up to the measure of the whole
    whole = as_dict(pctx.measure_field(v, *UNIT, shape, iso=0.25))
    assert P.sum_records([as_dict(m) for m in many.measures]) == {f: whole[f] for f in P.SHARED}


def test_two_runs_give_equal_bytes_on_any_stream(rm, pctx, crumbs):
    import torch
    shape, v, want, model = crumbs
    first = pctx.label_field(v, *UNIT, shape, iso=0.25, records=None)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = pctx.label_field(v, *UNIT, shape, iso=0.25, records=None)
        third = pctx.label_field(v.astype(np.float32), *UNIT, shape, iso=0.25, records=None, device=True)
    side.synchronize()
    assert first.labels.tobytes() == second.labels.tobytes() == want.tobytes()
    assert first.measures == second.measures and [as_dict(m) for m in second.measures] == model
    assert_parts(third, v.astype(np.float32), shape, 0.25, "inside", 1 << 20)


def test_select_meshes_the_kept_part_alone(rm, pctx):
    """Two spheres far apart: meshing the volume with the second mirrored away equals, byte for byte, meshing a volume that
    never held it -- the mirrored values lie on the outer side and no edge at the kept sphere has an end among them."""
    geom = box(-2.0, 2.0, (33, 33, 33))
    x = np.linspace(-2.0, 2.0, 33)
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    one = np.sqrt((xx + 0.9) ** 2 + y * y + z * z) - 0.6
    two = np.sqrt((xx - 1.1) ** 2 + (y - 0.5) ** 2 + z * z) - 0.4
    both = np.minimum(one, two)
    parts = pctx.label_field(both, *geom)
    assert parts.n_parts == 2 and parts.by_size() == [0, 1]
    kept = parts.select(both, [0])
    # where the second sphere was, the kept volume is positive as `one` is: same side everywhere, equal wherever a cell is active
    v_kept, q_kept = pctx.mesh_field(kept, *geom)
    v_one, q_one = pctx.mesh_field(one, *geom)
    assert len(v_one) > 0 and v_kept.tobytes() == v_one.tobytes() and q_kept.tobytes() == q_one.tobytes()
    v_both, _ = pctx.mesh_field(both, *geom)
    assert len(v_both) > len(v_one)
    # the same on the device
    import torch
    d_kept = parts.select(torch.from_numpy(both).cuda(), [0])
    assert d_kept.is_cuda and np.array_equal(d_kept.cpu().numpy(), kept)
