"""The numpy models at the shapes of tests/test_lattice_rounds_gpu.py, held to references that share nothing with them:
scipy.ndimage's labelling and distance transform, and sums in Python ints straight from the indices.  The models had only been
run at small shapes; the GPU tests take their word at large ones.  Also the guards that need no device: the workgroup and chunk
counts of the shapes against the header's constants.  Every comparison is equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edt_model as E  # noqa: E402
import measure_model as M  # noqa: E402
import parts_model as P  # noqa: E402
import rounds_volumes as V  # noqa: E402


def sets_of(shape):
    """The sets the GPU tests label and transform at a BIG shape: random ones on both sides, the two balls."""
    nu, nv, nw = shape
    for density in (0.31, 0.6):
        v = V.random_set_values(shape, density, np.float64)
        for side in (0, 1):
            yield "random %.2f side %d" % (density, side), P.in_set(v, nu, nv, nw, 0.25, side)
    yield "two balls", P.in_set(V.two_balls(shape), nu, nv, nw, 0.0)
    yield "few pieces", P.in_set(V.few_pieces(shape), nu, nv, nw, 0.0)


@pytest.mark.parametrize("shape", V.BIG)
def test_the_label_model_equals_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, s in sets_of(shape):
        found, count = ndimage.label(s, structure=ndimage.generate_binary_structure(3, 1))  # 6-connected
        flat = found.reshape(-1)
        # renumbered by smallest linear index, whatever order scipy numbers in
        ids, first = np.unique(flat, return_index=True)
        first = first[ids > 0]
        number = np.full(count + 1, -1, np.int64)
        number[ids[ids > 0][np.argsort(first)]] = np.arange(count)
        want = number[flat].reshape(s.shape).astype(np.int32)
        got = P.label(s)
        assert np.array_equal(got, want), (shape, name)
        assert P.info(s, got)["n_parts"] == count
    assert count == 3  # the few pieces came last


@pytest.mark.parametrize("shape", V.BIG)
def test_the_distance_model_equals_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, s in sets_of(shape):
        want = np.rint(ndimage.distance_transform_edt(s) ** 2).astype(np.int64)  # d2 <= 97^2 + 61^2 + 45^2: exact in binary64
        got = E.edt(s)
        assert np.array_equal(got, want), (shape, name)
        info = E.info(s, got)
        assert info["max_d2"] == int(want.max()) and info["argmax"] == int(np.argmax(want.reshape(-1)))


@pytest.mark.parametrize("shape", V.LONG)
def test_the_measure_model_equals_sums_in_python_ints(shape):
    nu, nv, nw = shape
    everywhere = np.full(V.size(shape), -1.0)
    for name, v, iso in (("random", V.random_measure_values(shape, np.float64), 0.25), ("two balls", V.two_balls(shape), 0.0),
                         ("all inside", everywhere, 0.0)):
        got = M.measure_dense(v, nu, nv, nw, iso)
        flat = np.asarray(v, np.float64).reshape(-1)
        inside = [bool(x < iso) for x in flat.tolist()]
        at = [(l % nu, l // nu % nv, l // (nu * nv)) for l, x in enumerate(inside) if x]
        assert got["n_points"] == nu * nv * nw and got["n_inside"] == len(at) > 0
        assert got["sum1"] == tuple(sum(p[c] for p in at) for c in range(3))
        assert got["sum2"] == tuple(sum(p[a] * p[b] for p in at) for a, b in M.PAIRS)
        assert got["lo"] == tuple(min(p[c] for p in at) for c in range(3)) and got["hi"] == tuple(max(p[c] for p in at) for c in range(3))
        stride, count = (1, nu, nu * nv), (nu, nv, nw)
        crossings = []
        for c in range(3):
            index = [l // stride[c] % count[c] for l in range(len(inside))]
            crossings.append(sum(1 for l, x in enumerate(inside) if index[l] + 1 < count[c] and inside[l + stride[c]] != x))
        assert got["crossings"] == tuple(crossings), (shape, name)
        assert got["n_nonfinite"] == (3 if name == "random" else 0)
    # all inside: the largest sums the shape can give
    most = max(shape) - 1
    assert max(got["hi"]) == most == 65534 and max(got["sum2"]) == (shape[0] * shape[1] * shape[2] // max(shape)) * most * (most + 1) * (2 * most + 1) // 6
    assert max(got["sum2"]) > 9 * 10 ** 13


def test_the_shapes_reach_the_second_rounds():
    block, step, reduce_most = V.constants()
    assert (block, V.WAVE) == (256, 64)
    assert [V.ceil_div(V.size(s), block) for s in V.BIG] == [1041, 1069] and min(1041, 1069) > max(step, reduce_most)
    assert [V.ceil_div(V.size(s), V.WAVE) for s in V.BIG] == [4161, 4274]
    assert V.BIG[1][0] == 4 * V.WAVE + 3
    assert V.ROWS[0][1] * V.ROWS[0][2] == 8777 and V.ceil_div(V.ROWS[1][0], V.FIELD_CHUNK) == 3 and V.ROWS[2][1] == 2
    assert [max(s) for s in V.LONG] == [65535] * 3 and [s.index(65535) for s in V.LONG] == [0, 1, 2]
    for shape in V.BIG:
        n_blocks = V.ceil_div(V.size(shape), block)
        # the disc lies in workgroups that edt_reduce_kernel's grid reaches in its second round only; its mirror image in the first
        l = np.flatnonzero(V.disc_at_the_end(shape, 6).reshape(-1) < 0)
        assert len(l) > 50 and l.min() // block >= reduce_most and (V.size(shape) - 1 - l.max()) // block < reduce_most
        assert n_blocks - reduce_most == (17 if shape == V.BIG[0] else 45)
        # the slabs: with two chunks a wave (a device of 129 to 260 CUs) some wave meets two single labels in succession
        labels = P.label(V.two_slabs(shape) < 0)
        assert int(labels.max()) == 1
        carried, changed, mixed = V.wave_paths(labels, 2, 2)
        assert carried > 0 and changed > 0 and mixed > 0, (shape, carried, changed, mixed)
        carried, changed, mixed = V.wave_paths(P.label(V.few_pieces(shape) < 0), 3, 2)
        assert carried > 0
