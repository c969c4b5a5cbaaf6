"""Distances on the GPU (rm_edt_field_device, rm_scene_edt, Context.edt_field / edt / open_field, Edt; include/rm_raymarch.h,
"distances").  d2 and the info are integers with one right answer: they must equal tests/edt_model.py's of the same values,
exactly.  No test provokes a fault or a hang."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_model as E  # noqa: E402
import parts_model as P  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, OCTREE, BVH = 0, 1, 2
INVALID, UNSUPPORTED, NO_SCENE = -1, -2, -5
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
SKEWED = ((-2.0, -2.05, 2.0), (0.125, 0.004, -0.003), (-0.005, 0.125, 0.006), (0.004, -0.003, -0.125), (33, 33, 33))
SIDES = ("inside", "outside")


def box(lo, hi, shape):
    """An axis-aligned lattice of `shape` points over [lo, hi]^3 (a count of 1: the plane at lo)."""
    step = [(hi - lo) / (n - 1) if n > 1 else 1.0 for n in shape]
    return ((lo, lo, lo), (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), shape)


BOX33 = box(-2.0, 2.0, (33, 33, 33))


def grid33():
    x = np.linspace(-2.0, 2.0, 33)
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    return xx, y, z


@pytest.fixture(scope="module")
def ectx(rm):
    """A context of its own.  Interpreter only, like the parts tests': every launch here is ahead-of-time."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    yield c
    c.close()


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def assert_edt(edt, values, shape, iso, side):
    """d2 and the info are the model's of `values`."""
    nu, nv, nw = shape
    s = P.in_set(values, nu, nv, nw, iso, SIDES.index(side))
    want = E.edt(s)
    d2 = host(edt.d2)
    assert d2.dtype == np.int32 and d2.shape == (nw, nv, nu)
    assert np.array_equal(d2, want), (shape, side)
    info = E.info(s, want)
    assert dict(n_points=edt.n_points, n_set=edt.n_set, max_d2=edt.max_d2, argmax=edt.argmax) == info, (shape, side)
    assert edt.side == side
    return s, want


def random_values(rng, n, density, dtype):
    """The parts tests' recipe: values about iso = 0.25 of which `density` lie below; some equal iso, one NaN, both infinities."""
    v = rng.random(n) - density + 0.25
    if n >= 16:
        v[::7] = 0.25
        v[3], v[5], v[9] = float("nan"), float("inf"), float("-inf")
    return v.astype(dtype)


def kernel_of(shape):
    return "edt_axis_kernel" if shape[1] > 1 or shape[2] > 1 else "edt_rows_kernel"


# (67, 10, 21): a row longer than a wave and no multiple of 64 -- rows that begin and end inside a wave, rows that leave it on
# either side --; rows of one, two and four waves and one point more; planes and lines; a single point; no point
SHAPES = [(67, 10, 21), (130, 5, 3), (64, 4, 4), (65, 4, 4), (256, 3, 2), (1, 1, 1), (1, 9, 9), (9, 1, 9), (9, 9, 1), (5, 0, 3)]


@pytest.mark.parametrize("shape", SHAPES)
def test_random_volumes_equal_the_model(rm, ectx, shape):
    nu, nv, nw = shape
    n = nu * nv * nw
    rng = np.random.default_rng(nu + 7 * nv)
    before = ectx.last_kernel()
    for density in (0.2, 0.5, 0.9, 0.999, 1.0, 0.0):  # 1.0: all in, 0.0: all out
        for dtype in (np.float64, np.float32):
            v = random_values(rng, n, density, dtype)
            if density in (1.0, 0.0):
                v = np.full(n, 0.0 if density else 1.0, dtype)
            for side in SIDES:
                edt = ectx.edt_field(v, *UNIT, shape, iso=0.25, side=side)
                assert_edt(edt, v, shape, 0.25, side)
                assert ectx.last_kernel() == (kernel_of(shape) if n else before)
                if n and (density, side) in ((1.0, "inside"), (0.0, "outside")):  # the whole lattice in the set
                    assert (edt.d2 == E.FAR).all() and (edt.max_d2, edt.argmax, edt.n_set) == (E.FAR, 0, n)
    if n == 0:
        assert (edt.n_points, edt.n_set, edt.max_d2, edt.argmax, edt.at) == (0, 0, 0, -1, None)


FAR_SHAPES = [(67, 10, 21), (3, 300, 2), (2, 3, 300)]  # the last two: long lines along j and along k


@pytest.mark.parametrize("shape", FAR_SHAPES)
def test_one_parabola_wins_a_whole_volume(rm, ectx, shape):
    import torch
    nu, nv, nw = shape
    far_faces = [(nu - 1, nv // 2, nw // 2), (nu // 2, nv - 1, nw // 2), (nu // 2, nv // 2, nw - 1)]
    for name, outside in (("corner", [(0, 0, 0)]), ("centre", [(nu // 2, nv // 2, nw // 2)]), ("far faces", far_faces),
                          ("far corner", [(nu - 1, nv - 1, nw - 1)])):
        v = np.full((nw, nv, nu), -1.0)
        for i, j, k in outside:
            v[k, j, i] = 1.0
        edt = ectx.edt_field(torch.from_numpy(v).cuda(), *UNIT, shape, device=True)
        assert edt.d2.is_cuda
        assert_edt(edt, v, shape, 0.0, "inside")
        assert ectx.last_kernel() == "edt_axis_kernel"
        if name == "corner":
            assert edt.max_d2 == (nu - 1) ** 2 + (nv - 1) ** 2 + (nw - 1) ** 2 and edt.at == (nu - 1, nv - 1, nw - 1)
            if shape == (67, 10, 21):
                assert edt.max_d2 == 66 ** 2 + 9 ** 2 + 20 ** 2
        if name == "far corner":
            assert edt.max_d2 == (nu - 1) ** 2 + (nv - 1) ** 2 + (nw - 1) ** 2 and edt.argmax == 0


def raw_edt(rm, ctx, lat, values, vt, iso, side, d2, info, stream=None):
    """rm_edt_field_device through ctypes; tensors or None."""
    import torch
    N = rm._native
    ptr = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    return N.lib().rm_edt_field_device(ctx._h, C.byref(lat), ptr(values), vt, float(iso), side, ptr(d2), ptr(info),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream)


def test_the_longest_line_and_the_range_refusal(rm, ectx):
    import torch
    n = 46341
    i = np.arange(n, dtype=np.int64)
    v = np.full(n, -1.0)
    v[0] = 1.0
    edt = ectx.edt_field(v, *UNIT, (n, 1, 1))
    assert edt.d2.shape == (1, 1, n) and np.array_equal(edt.d2.reshape(-1), i * i)
    assert (edt.n_set, edt.max_d2, edt.argmax) == (n - 1, 46340 ** 2, 46340) and ectx.last_kernel() == "edt_rows_kernel"
    # the other way: every wave but the last finds its point of T behind it
    edt = ectx.edt_field(v[::-1].copy(), *UNIT, (n, 1, 1))
    assert np.array_equal(edt.d2.reshape(-1), (i * i)[::-1]) and (edt.max_d2, edt.argmax) == (46340 ** 2, 0)
    # and as a line along j and along k: one lane walks it
    for shape in ((1, n, 1), (1, 1, n)):
        edt = ectx.edt_field(v, *UNIT, shape)
        assert np.array_equal(edt.d2.reshape(-1), i * i) and (edt.max_d2, edt.argmax) == (46340 ** 2, 46340)
        assert ectx.last_kernel() == "edt_axis_kernel"
    # one point more does not fit; neither does a wide plane of fewer than 2^30 points.  Refused ahead of any launch: the
    # pointers are never read.  A bad side is refused first.
    some = torch.zeros(64, dtype=torch.float64, device="cuda")
    d2 = torch.zeros(64, dtype=torch.int32, device="cuda")
    info = torch.zeros(4, dtype=torch.int64, device="cuda")
    for shape in ((46342, 1, 1), (1, 46342, 1), (40000, 26000, 1)):
        lat = rm.make_lattice(*UNIT, shape=shape)
        assert raw_edt(rm, ectx, lat, some, 0, 0.0, 0, d2, info) == UNSUPPORTED
        assert raw_edt(rm, ectx, lat, some, 0, 0.0, 2, d2, info) == INVALID
        assert raw_edt(rm, ectx, lat, some, 0, 0.0, 0, d2, None) == INVALID
    with pytest.raises(rm.RmUnsupported):
        ectx.edt_field(np.zeros(46342), *UNIT, (46342, 1, 1))
    torch.cuda.synchronize()
    assert not d2.any() and not info.any()


def test_nothing_behind_the_buffers_is_written_and_every_info_field_is(rm, ectx):
    import torch
    shape = (67, 10, 21)
    n = 67 * 10 * 21
    lat = rm.make_lattice(*UNIT, shape=shape)
    v = random_values(np.random.default_rng(31), n, 0.6, np.float64)
    values = torch.from_numpy(v).cuda()
    s = P.in_set(v, *shape, 0.25)
    want = E.edt(s)
    model = E.info(s, want)
    guard = 256
    d2 = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    info = torch.full((4 + guard,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")  # 0xA5 bytes
    assert (info.cpu().numpy().view(np.uint8) == 0xA5).all()
    assert raw_edt(rm, ectx, lat, values, 0, 0.25, 0, d2, info) == 0
    got, head = d2.cpu().numpy(), info.cpu().numpy()
    assert np.array_equal(got[:n], want.reshape(-1)) and (got[n:] == 0x5A5A5A5A).all()
    assert head[:4].tolist() == [model["n_points"], model["n_set"], model["max_d2"], model["argmax"]]
    assert (head[4:].view(np.uint8) == 0xA5).all()
    # a lattice without points writes the info alone -- {0, 0, 0, -1} -- and asks for neither values nor d2
    info.fill_(-0x5A5A5A5A5A5A5A5B)
    before = ectx.last_kernel()
    assert raw_edt(rm, ectx, rm.make_lattice(*UNIT, shape=(5, 0, 3)), None, 0, 0.25, 0, None, info) == 0
    head = info.cpu().numpy()
    assert head[:4].tolist() == [0, 0, 0, -1] and (head[4:].view(np.uint8) == 0xA5).all() and ectx.last_kernel() == before
    # null and misaligned pointers
    assert raw_edt(rm, ectx, lat, None, 0, 0.25, 0, d2, info) == INVALID
    assert raw_edt(rm, ectx, lat, values, 0, 0.25, 0, None, info) == INVALID
    assert raw_edt(rm, ectx, lat, values, 0, 0.25, 0, d2, None) == INVALID
    assert raw_edt(rm, ectx, lat, values.data_ptr() + 4, 0, 0.25, 0, d2, info) == INVALID
    assert raw_edt(rm, ectx, lat, values, 0, 0.25, 0, d2.data_ptr() + 2, info) == INVALID
    assert raw_edt(rm, ectx, lat, values, 0, 0.25, 0, d2, info.data_ptr() + 4) == INVALID
    torch.cuda.synchronize()
    assert np.array_equal(d2.cpu().numpy(), got)


def test_two_runs_give_equal_bytes_on_any_stream(rm, ectx):
    import torch
    shape = (67, 10, 21)
    v = random_values(np.random.default_rng(31), 67 * 10 * 21, 0.6, np.float64)
    first = ectx.edt_field(v, *UNIT, shape, iso=0.25)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = ectx.edt_field(v, *UNIT, shape, iso=0.25)
        third = ectx.edt_field(v.astype(np.float32), *UNIT, shape, iso=0.25, device=True)
    side.synchronize()
    s, want = assert_edt(first, v, shape, 0.25, "inside")
    assert first.d2.tobytes() == second.d2.tobytes() == want.tobytes()
    assert (first.n_set, first.max_d2, first.argmax) == (second.n_set, second.max_d2, second.argmax)
    assert_edt(third, v.astype(np.float32), shape, 0.25, "inside")


def scene_edt(rm, ctx, geom, iso, side, want_d2=True):
    """rm_scene_edt through ctypes, every output filled with 0xA5 bytes first."""
    N = rm._native
    lat = rm.make_lattice(*geom)
    n = lat.nu * lat.nv * lat.nw
    d2 = np.full(n, -1515870811, np.int32)
    info = N.rm_edt_info()
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    N.check(ctx._h, N.lib().rm_scene_edt(ctx._h, C.byref(lat), float(iso), SIDES.index(side), d2.ctypes.data_as(C.c_void_p) if want_d2 else None,
                                         C.byref(info)))
    return d2.reshape(lat.nw, lat.nv, lat.nu), info


def test_one_sphere_has_its_radius_for_an_inradius(rm, ectx):
    results = []
    for accel in (BVH, OCTREE):
        ectx.scene_from_preset(0, accel)  # one sphere of radius 1.5 about the origin
        edt = ectx.edt(*BOX33)
        assert (edt.max_d2, edt.argmax, edt.at) == (144, 17968, (16, 16, 16)) and edt.step == 0.125 and edt.inradius == 1.5
        assert edt.distance()[16, 16, 16] == 1.5 and edt.distance().dtype == np.float64
        vol, _ = ectx.field(*BOX33, count=False, device=True, exact=True)
        assert_edt(edt, vol.cpu().numpy(), BOX33[4], 0.0, "inside")
        d2, info = scene_edt(rm, ectx, BOX33, 0.0, "inside")
        assert np.array_equal(d2, edt.d2)
        assert (info.n_points, info.n_set, info.max_d2, info.argmax) == (33 ** 3, edt.n_set, 144, 17968)
        _, info = scene_edt(rm, ectx, BOX33, 0.0, "inside", want_d2=False)
        assert (info.n_set, info.max_d2, info.argmax) == (edt.n_set, 144, 17968)
        assert ectx.last_kernel() == "edt_axis_kernel"
        results.append(edt.d2.tobytes())
    assert results[0] == results[1]  # the exact field does not depend on the structure
    sc = rm.Scene("BVH", ctx=ectx)
    sc.loadPreset(0)
    assert sc.edt(*BOX33).d2.tobytes() == results[0]
    boxed = sc.edt(cells=(20, 20, 20))
    assert boxed.n_points == 21 ** 3 and boxed.d2.shape == (21, 21, 21) and boxed.step is not None and boxed.max_d2 < E.FAR
    # the margin keeps the sphere off the border.  The lattice point nearest the centre is within sqrt(3) / 2 steps of it, and a
    # lattice point outside the sphere lies within sqrt(3) steps of any point of its surface
    assert 1.5 - boxed.step <= boxed.inradius <= 1.5 + 3 * boxed.step
    assert ectx.get_option("exact") == 0
    # a lattice without points: the info alone
    _, info = scene_edt(rm, ectx, box(-2.0, 2.0, (5, 0, 3)), 0.0, "inside")
    assert (info.n_points, info.n_set, info.max_d2, info.argmax) == (0, 0, 0, -1)
    # without a scene the entry says so, behind its argument checks
    with rm.Context(0) as empty:
        N = rm._native
        lat = rm.make_lattice(*BOX33)
        inf = N.rm_edt_info()
        assert N.lib().rm_scene_edt(empty._h, C.byref(lat), 0.0, 0, None, C.byref(inf)) == NO_SCENE
        assert N.lib().rm_scene_edt(empty._h, C.byref(lat), 0.0, 3, None, C.byref(inf)) == INVALID
        assert N.lib().rm_scene_edt(empty._h, C.byref(rm.make_lattice(*UNIT, shape=(46342, 1, 1))), 0.0, 0, None, C.byref(inf)) == UNSUPPORTED


def test_inside_a_union_the_exact_field_is_not_the_distance(rm, ectx):
    centres = np.array([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]], np.float32)
    ectx.scene_from_spheres(centres, np.array([1.0, 1.0]), BVH)
    edt = ectx.edt(*BOX33)
    vol, _ = ectx.field(*BOX33, count=False, device=True, exact=True)
    vol = vol.cpu().numpy().reshape(33, 33, 33)
    assert vol[16, 16, 16] == -0.5  # 4 cells, says the minimum over the spheres
    assert edt.d2[16, 16, 16] == 49 and edt.distance()[16, 16, 16] == 7.0 * 0.125  # 7 cells to the union's surface
    assert_edt(edt, vol, BOX33[4], 0.0, "inside")


def neck():
    """Two spheres of radius 0.6 at x = +-0.9 joined by a cylinder of radius 0.2."""
    x, y, z = grid33()
    one = np.sqrt((x + 0.9) ** 2 + y * y + z * z) - 0.6
    two = np.sqrt((x - 0.9) ** 2 + y * y + z * z) - 0.6
    rod = np.maximum(np.hypot(y, z) - 0.2, np.abs(x) - 0.9)
    return np.minimum(np.minimum(one, two), rod)


def test_erosion_finds_a_neck_and_the_opening_removes_it(rm, ectx):
    import torch
    v = neck()
    shape = BOX33[4]
    edt = ectx.edt_field(v, *BOX33)
    s, want = assert_edt(edt, v, shape, 0.0, "inside")
    whole = ectx.label_field(v, *BOX33)
    assert whole.n_parts == 1 and whole.n_set == edt.n_set == int(s.sum())
    counts = {}
    for r2 in (4, 5):
        eroded = edt.eroded(r2)
        assert eroded.dtype == np.float64 and np.array_equal(eroded, E.eroded(s, want, r2))
        parts = ectx.label_field(eroded, *BOX33)
        assert np.array_equal(parts.labels, P.label(eroded < 0))
        counts[r2] = parts.n_parts
    assert counts == {4: 1, 5: 2}  # the neck is between 2 and sqrt(5) cells thick: the assertion that matters
    assert parts.n_set == int((E.eroded(s, want, 5) < 0).sum())
    assert np.array_equal(edt.max_by_part(parts), E.max_by_part(want, parts.labels)) and edt.max_by_part(parts).dtype == np.int64
    assert edt.max_by_part(parts).max() == edt.max_d2 == int(want.max())
    # the same on the device
    dev = ectx.edt_field(torch.from_numpy(v).cuda(), *BOX33, device=True)
    d_eroded = dev.eroded(5)
    assert d_eroded.is_cuda and d_eroded.dtype == torch.float64 and np.array_equal(d_eroded.cpu().numpy(), eroded)
    d_parts = ectx.label_field(d_eroded, *BOX33, device=True)
    d_most = dev.max_by_part(d_parts)
    assert d_most.is_cuda and d_most.dtype == torch.int64 and np.array_equal(d_most.cpu().numpy(), edt.max_by_part(parts))
    # the opening: two parts, none of it outside the original
    opened = ectx.open_field(v, *BOX33, r2=5)
    assert opened.dtype == np.float64 and opened.shape == (33, 33, 33) and np.array_equal(opened, E.opened(s, 5))
    assert ((opened < 0) <= s).all() and int((opened < 0).sum()) < int(s.sum())
    assert ectx.label_field(opened, *BOX33).n_parts == 2
    d_opened = ectx.open_field(torch.from_numpy(v).cuda(), *BOX33, r2=5, device=True)
    assert d_opened.is_cuda and np.array_equal(d_opened.cpu().numpy(), opened)
    # the figures of this construction
    assert (edt.n_set, edt.max_d2, parts.n_set, int((opened < 0).sum())) == (959, 22, 230, 910)


def test_a_shell_from_the_outside_and_distances_need_a_cubic_lattice(rm, ectx):
    x, y, z = grid33()
    r = np.sqrt(x * x + y * y + z * z)
    v = np.abs(r - 1.0) - 0.2
    outside = ectx.edt_field(v, *BOX33, side="outside")
    s, want = assert_edt(outside, v, BOX33[4], 0.0, "outside")
    shell = v < 0
    assert (outside.d2[shell] == 0).all() and (outside.d2[~shell] > 0).all()
    assert outside.d2[16, 16, 16] > 0 and outside.d2[0, 0, 0] > 0  # the void and the surroundings
    inside = ectx.edt_field(v, *BOX33)
    assert inside.n_set + outside.n_set == 33 ** 3 and ((inside.d2 > 0) == shell).all()
    assert outside.step == 0.125 and np.array_equal(outside.distance(), np.sqrt(want.astype(np.float64)) * 0.125)
    skewed = ectx.edt_field(v, *SKEWED, side="outside")
    assert skewed.step is None and np.array_equal(skewed.d2, outside.d2)  # index units: the steps are not read
    with pytest.raises(ValueError):
        skewed.distance()
    with pytest.raises(ValueError):
        skewed.inradius
