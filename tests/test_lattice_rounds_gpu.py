"""The lattice kernels past one round (rm_measure.hip, rm_parts.hip, rm_edt.hip): lattices large enough that a wave of
measure_field_kernel takes a second row and a second pair of chunks, parts_scan_kernel and edt_reduce_kernel a second step,
a wave of parts_measure_kernel a second chunk with its sums carried, the row carries of edt_rows_kernel several segments, and the
closed forms of the measure's dropped blocks base indices near 2^16.  Every test first asserts, from the header's constants, the
lattice and the device's CU count -- never from the code under test --, that its input reaches the loop it is meant for.  Every
quantity is an integer with one right answer: the results must equal tests/measure_model.py's, parts_model.py's and
edt_model.py's of the same values, which tests/test_lattice_rounds.py holds to scipy at these shapes.  No tolerance anywhere; no
test provokes a fault or a hang."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_model as E  # noqa: E402
import measure_model as M  # noqa: E402
import parts_model as P  # noqa: E402
import rounds_volumes as V  # noqa: E402

pytestmark = pytest.mark.gpu

BVH = 2
UNIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
SIDES = ("inside", "outside")
ALL_RECORDS = 1 << 20


@pytest.fixture(scope="module")
def lctx(rm):
    """A context of its own.  Interpreter only, like the measure tests': every launch here is ahead-of-time."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def as_dict(m):
    return dict(m._asdict())


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


# ------------------------------------------------------------------------------------------------- measures, dense

# which loops of measure_field_kernel a shape is there for: "rows" -- a wave takes a second row: the grid has at most 8 workgroups
# of 4 waves a CU --, "chunks" -- a row is more than one step of 128 points
MEASURE_REACHES = {V.BIG[0]: (), V.BIG[1]: ("chunks",), V.ROWS[0]: ("rows",), V.ROWS[1]: ("chunks",), V.ROWS[2]: ("rows",),
                   V.LONG[0]: ("chunks",), V.LONG[1]: ("rows", "no step along k"), V.LONG[2]: ("rows", "no step along j")}


@pytest.mark.parametrize("shape", V.BIG + V.ROWS + V.LONG)
def test_measures_of_many_rows_and_long_rows_equal_the_model(rm, lctx, cus, shape):
    nu, nv, nw = shape
    reaches = MEASURE_REACHES[shape]
    if "rows" in reaches:
        assert nv * nw > 32 * cus, (shape, cus)
    if "chunks" in reaches:
        assert nu > V.FIELD_CHUNK
    if "no step along k" in reaches:  # the stride over the rows is below nv: k moves by the wrap alone
        assert nv > 32 * cus
    if "no step along j" in reaches:
        assert nv == 1
    volumes = [("random", V.random_measure_values(shape, np.float64), 0.25), ("two balls", V.two_balls(shape), 0.0)]
    if shape in V.LONG:  # the largest sums the shape can give
        volumes.append(("all inside", np.full(V.size(shape), -1.0), 0.0))
    for name, v, iso in volumes:
        for dtype in (np.float64, np.float32):
            values = v.astype(dtype)
            got = lctx.measure_field(values, *UNIT, shape, iso=iso)
            want = M.measure_dense(values, nu, nv, nw, iso)
            assert as_dict(got) == want, (shape, name, dtype.__name__, got, want)
            assert lctx.last_kernel() == "measure_field_kernel<%s>" % ("float" if dtype is np.float32 else "double")
            assert got.n_inside > 0 and got.n_nonfinite == (3 if name == "random" else 0)
            if name == "all inside":
                assert got.n_inside == nu * nv * nw and got.lo == (0, 0, 0) and got.hi == (nu - 1, nv - 1, nw - 1)
                assert max(got.sum2) > 9 * 10 ** 13


# ------------------------------------------------------------------------------------------------- parts

def assert_parts(parts, values, shape, iso, side, records):
    """Labels, info and the first `records` records are the model's of `values` (tests/test_parts_gpu.py's check).  That the
    entry returned at all says gave_up == 0: Context.label_field raises otherwise."""
    nu, nv, nw = shape
    s = P.in_set(values, nu, nv, nw, iso, SIDES.index(side))
    want = P.label(s)
    labels = host(parts.labels)
    assert labels.dtype == np.int32 and labels.shape == (nw, nv, nu)
    assert np.array_equal(labels, want), (shape, side)
    info = P.info(s, want)
    assert (parts.n_points, parts.n_set, parts.n_parts) == (info["n_points"], info["n_set"], info["n_parts"]), (shape, side)
    model = P.part_records(want, min(records, info["n_parts"]))
    assert [as_dict(m) for m in parts.measures] == model, (shape, side)
    return want, model


def assert_records_add_up(lctx, parts, values, shape, iso):
    whole = as_dict(lctx.measure_field(values, *UNIT, shape, iso=iso))
    assert P.sum_records([as_dict(m) for m in parts.measures]) == {f: whole[f] for f in P.SHARED}, shape


def per_wave(shape, cus):
    """The chunks a wave of parts_measure_kernel takes: its grid is 16 waves a CU at most."""
    chunks = V.ceil_div(V.size(shape), V.WAVE)
    assert chunks > 16 * cus, (shape, cus)
    return V.ceil_div(chunks, 16 * cus)


def assert_scan_steps(shape):
    block, step, _ = V.constants()
    assert V.ceil_div(V.size(shape), block) > step
    return block * step  # the first point whose workgroup the scan reaches in its second step


@pytest.mark.parametrize("shape", V.BIG)
def test_random_parts_are_numbered_across_scan_steps(rm, lctx, cus, shape):
    second_step = assert_scan_steps(shape)
    per_wave(shape, cus)
    for density in (0.31, 0.6):
        v = V.random_set_values(shape, density, np.float64)
        for side in SIDES:
            parts = lctx.label_field(v, *UNIT, shape, iso=0.25, side=side, records=None)
            want, _ = assert_parts(parts, v, shape, 0.25, side, ALL_RECORDS)
            assert len(parts.measures) == parts.n_parts and lctx.last_kernel() == "parts_measure_kernel"
            # a part whose root lies in a workgroup of the scan's second step: its number is an offset that crossed the step
            assert np.flatnonzero(want.reshape(-1) == parts.n_parts - 1)[0] >= second_step
            if side == "inside":
                assert parts.n_parts > (10000 if density < 0.5 else 100)
                assert_records_add_up(lctx, parts, v, shape, 0.25)
    v = V.random_set_values(shape, 0.31, np.float32, seed=1)
    parts = lctx.label_field(v, *UNIT, shape, iso=0.25, records=None, device=True)
    assert_parts(parts, v, shape, 0.25, "inside", ALL_RECORDS)
    assert_records_add_up(lctx, parts, v, shape, 0.25)


@pytest.mark.parametrize("shape", V.BIG)
def test_a_solid_in_few_pieces_carries_its_sums_from_chunk_to_chunk(rm, lctx, cus, shape):
    assert_scan_steps(shape)
    span = per_wave(shape, cus)
    v = V.few_pieces(shape)
    for side in SIDES:
        parts = lctx.label_field(v, *UNIT, shape, side=side, records=None)
        want, _ = assert_parts(parts, v, shape, 0.0, side, ALL_RECORDS)
        carried, _, _ = V.wave_paths(want, parts.n_parts, span)
        assert carried > 0 and parts.n_parts == (3 if side == "inside" else 1)
    parts = lctx.label_field(v, *UNIT, shape, records=None)
    assert_records_add_up(lctx, parts, v, shape, 0.0)
    assert parts.measures[2].n_inside == 12 and parts.measures[2].lo == (2, 2, shape[2] - 3)
    # one record: the points of the other two parts are in the set and have none
    one = lctx.label_field(v, *UNIT, shape, records=1)
    want, model = assert_parts(one, v, shape, 0.0, "inside", 1)
    assert len(one.measures) == 1 and one.n_parts == 3 and as_dict(one.measures[0]) == as_dict(parts.measures[0])
    assert V.wave_paths(want, 1, span)[0] > 0 and V.wave_paths(want, 3, span)[0] > V.wave_paths(want, 1, span)[0]


@pytest.mark.parametrize("shape", V.BIG)
def test_two_slabs_change_the_label_between_the_chunks_of_a_wave(rm, lctx, cus, shape):
    span = per_wave(shape, cus)
    v = V.two_slabs(shape)
    for side in SIDES:
        parts = lctx.label_field(v, *UNIT, shape, side=side, records=None)
        want, _ = assert_parts(parts, v, shape, 0.0, side, ALL_RECORDS)
        if side == "inside":
            # a wave meets one label alone and then the other alone -- it sends its sums and starts again --, and chunks of both
            carried, changed, mixed = V.wave_paths(want, 2, span)
            assert parts.n_parts == 2 and carried > 0 and changed > 0 and mixed > 0, (shape, span, carried, changed, mixed)
            assert_records_add_up(lctx, parts, v, shape, 0.0)
        else:
            assert parts.n_parts == 3  # the wall and the two strips at the seams
    v32 = v.astype(np.float32)
    assert_parts(lctx.label_field(v32, *UNIT, shape, records=None), v32, shape, 0.0, "inside", ALL_RECORDS)


# ------------------------------------------------------------------------------------------------- distances

def assert_edt(edt, values, shape, iso, side):
    """d2 and the info are the model's of `values` (tests/test_edt_gpu.py's check)."""
    nu, nv, nw = shape
    s = P.in_set(values, nu, nv, nw, iso, SIDES.index(side))
    want = E.edt(s)
    d2 = host(edt.d2)
    assert d2.dtype == np.int32 and d2.shape == (nw, nv, nu)
    assert np.array_equal(d2, want), (shape, side)
    info = E.info(s, want)
    assert dict(n_points=edt.n_points, n_set=edt.n_set, max_d2=edt.max_d2, argmax=edt.argmax) == info, (shape, side)
    return s, want


def assert_reduce_rounds(shape):
    block, _, most = V.constants()
    assert V.ceil_div(V.size(shape), block) > most
    return block, most


@pytest.mark.parametrize("shape", V.BIG)
def test_random_distances_break_ties_across_the_rounds_of_the_reduction(rm, lctx, shape):
    block, most = assert_reduce_rounds(shape)
    for density in (0.5, 0.9):
        v = V.random_set_values(shape, density, np.float64)
        for side in SIDES:
            edt = lctx.edt_field(v, *UNIT, shape, iso=0.25, side=side)
            s, want = assert_edt(edt, v, shape, 0.25, side)
            assert lctx.last_kernel() == "edt_axis_kernel"
            ties = np.flatnonzero(want.reshape(-1) == edt.max_d2)
            assert edt.argmax == ties[0]
            if (density, side) == (0.9, "inside"):
                # the largest d2 is taken more than once, also in a workgroup of the second round: the smallest index has to win
                assert len(ties) > 1 and ties[-1] // block >= most > ties[0] // block, (shape, ties)
    v = V.random_set_values(shape, 0.9, np.float32, seed=1)
    assert_edt(lctx.edt_field(v, *UNIT, shape, iso=0.25, device=True), v, shape, 0.25, "inside")


@pytest.mark.parametrize("shape", V.BIG)
def test_distances_of_balls_and_of_a_solid_in_the_last_workgroups(rm, lctx, shape):
    block, most = assert_reduce_rounds(shape)
    # long envelope stacks: d2 up to about 100
    balls = V.two_balls(shape)
    for side in SIDES:
        edt = lctx.edt_field(balls, *UNIT, shape, side=side)
        assert_edt(edt, balls, shape, 0.0, side)
        assert side == "outside" or edt.max_d2 >= 36
    # the only points of the set lie in workgroups of the reduction's second round; mirrored: of its first; then in both
    disc = V.disc_at_the_end(shape, 6)
    mirrored = disc[::-1, ::-1, ::-1].copy()
    both = np.minimum(disc, mirrored)
    n = V.size(shape)
    l = np.flatnonzero(disc.reshape(-1) < 0)
    assert len(l) > 50 and l.min() // block >= most and (n - 1 - l.max()) // block < most
    for name, v, first in (("last", disc, int(l.min())), ("first", mirrored, n - 1 - int(l.max())), ("both", both, n - 1 - int(l.max()))):
        edt = lctx.edt_field(v, *UNIT, shape)
        assert_edt(edt, v, shape, 0.0, "inside")
        # one plane thick: d2 = 1 all over the disc, and the first of its points is the argmax
        assert (edt.n_set, edt.max_d2, edt.argmax) == (len(l) * (2 if name == "both" else 1), 1, first), (shape, name)
        assert_edt(lctx.edt_field(v, *UNIT, shape, side="outside"), v, shape, 0.0, "outside")


def test_row_carries_walk_several_segments(rm, lctx):
    """(259, 33, 32): the only point outside the set is the first (the last) of every row, so the nearest one lies in the
    point's own row, d2 = i^2 ((258 - i)^2), and a wave at the far end of a row walks three further segments to find it."""
    shape = V.BIG[1]
    nu = shape[0]
    assert nu - 1 > 4 * V.WAVE
    i = np.arange(nu, dtype=np.int64)
    for last, along in ((False, i * i), (True, (nu - 1 - i) ** 2)):
        v = V.row_ends(shape, last)
        edt = lctx.edt_field(v, *UNIT, shape)
        assert_edt(edt, v, shape, 0.0, "inside")
        assert (edt.d2 == along.reshape(1, 1, nu)).all() and edt.max_d2 == (nu - 1) ** 2
        assert edt.argmax == (0 if last else nu - 1)
        assert_edt(lctx.edt_field(v.astype(np.float32), *UNIT, shape, side="outside"), v.astype(np.float32), shape, 0.0, "outside")


# ------------------------------------------------------------------------------------------------- measures, sparse

def test_dropped_blocks_at_large_base_indices_take_the_closed_forms(rm, lctx):
    """Preset 0 over (9, 9, 65529), x, y in [-0.2, 0.2], z in [-1, 2]: 8 191 blocks along k.  Those below the sphere's top are
    dropped as inside and take the closed forms at base indices up to some 48 000; those about z = 1.5 are kept, their tiles
    join base indices up to some 61 000; the rest is dropped as outside."""
    lctx.scene_from_preset(0, BVH)
    nu, nv, nw = V.SPARSE[4]
    sparse = lctx.measure(*V.SPARSE)
    assert lctx.last_kernel() == "measure_tiles_kernel"
    vol, _ = lctx.field(*V.SPARSE, count=False, device=True, exact=True)
    dense = lctx.measure_field(vol, *V.SPARSE)
    want = M.measure_dense(vol.cpu().numpy(), nu, nv, nw, 0.0)
    # the input reaches large base indices: by the model, the solid spans k = 0 .. beyond 50 000
    assert want["lo"][2] == 0 and want["hi"][2] > 50000 and want["sum2"][2] > 10 ** 15
    assert as_dict(dense) == want
    assert M.same_measure(as_dict(sparse), as_dict(dense)), (sparse, dense)
    assert sparse.n_blocks == (nw + 6) // 8 == 8191 and 0 < sparse.n_kept < sparse.n_blocks
    assert sparse.n_blocks_inside > 4000 and sparse.n_kept + sparse.n_blocks_inside < sparse.n_blocks
    assert as_dict(lctx.measure(*V.SPARSE, sparse=False, exact=True)) == as_dict(dense)
