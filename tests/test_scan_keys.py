"""The three-key update of the one-radius scan (rm_kernels.h rm_scan_keys_update: the text scan_sphere<true> of the v2 wave loop
runs), on the CPU through rm_debug_scan_keys.

A key is the bit pattern of a squared centre distance with the sphere's id in its low byte.  After a scan the three keys hold the
three smallest that were fed, in order, equal keys counted as often as they came, all ones where there were fewer; the third
key's bound (`lb3` of section M's runner-up test) is +inf exactly when fewer than three spheres were scanned.  The reference is a
sort of the same keys."""
import numpy as np
import pytest

from cpu_raymarcher_amd.context import Context

NONE = 0xFFFFFFFF
F = np.float32


def key(s2, ident):
    return (int(np.array(s2, F).view(np.uint32)) & 0xFFFFFF00) | ident


def expected(keys):
    return (sorted(int(k) for k in keys) + [NONE] * 3)[:3]


def run(keys, rf=0.15):
    got, lb3, carried = Context.scan_keys(np.array(keys, np.uint32), rf)
    assert got == expected(keys), (keys, got)
    # what section M reads never exceeds the bound, and gives away at most 3 % of a positive one
    assert carried <= lb3 and (carried >= 0.97 * lb3 if lb3 >= 0 else carried >= 1.03 * lb3), (keys, lb3, carried)
    assert np.isinf(lb3) == (len(keys) < 3) and not np.isnan(lb3), (keys, lb3)
    if len(keys) >= 3:  # the bound is scan_finish_uniform's formula on the third key's squared distance, the id byte cleared
        length = float(np.sqrt(np.array(got[2] & 0xFFFFFF00, np.uint32).view(F)))
        want = (length - rf) - (length + abs(rf) + 1.0) * 4e-6
        assert abs(lb3 - want) <= 1e-6 * (1.0 + abs(want)), (keys, lb3, want)
    return got, lb3


@pytest.mark.parametrize("n", [0, 1, 2, 3, 40])
def test_three_smallest_of_n_keys_in_every_order_tried(n):
    rng = np.random.default_rng(100 + n)
    keys = [key(s, i) for i, s in enumerate(rng.uniform(0.0, 9.0, n))]
    run(keys)
    run(sorted(keys))
    run(sorted(keys, reverse=True))
    for _ in range(20):
        run(list(rng.permutation(np.array(keys, np.uint64))))


def test_equal_keys_count_as_separate_spheres():
    a, b, c = key(1.0, 7), key(2.0, 3), key(4.0, 9)
    assert run([a, a])[0] == [a, a, NONE]
    assert run([a, a, a])[0] == [a, a, a]
    assert run([b, a, a])[0] == [a, a, b]
    assert run([a, b, b, c])[0] == [a, b, b]
    assert run([c, b, a, c, b, a])[0] == [a, a, b]
    assert run([c] * 40)[0] == [c, c, c]


def test_keys_equal_in_all_but_the_id_byte():
    keys = [key(2.25, i) for i in (200, 3, 255, 0, 77)]
    got, lb3 = run(keys)
    assert [k & 0xFF for k in got] == [0, 3, 77] and len({k >> 8 for k in got}) == 1
    assert lb3 == run([key(2.25, 0)] * 3)[1]  # the id byte takes no part in the bound


def test_the_all_ones_initial_value():
    assert run([])[0] == [NONE, NONE, NONE]
    a = key(0.0, 0)
    assert run([a])[0] == [a, NONE, NONE]
    # all ones fed as a key is "no sphere" again: it orders behind every key of a finite distance
    got, lb3, carried = Context.scan_keys(np.array([NONE, a, NONE], np.uint32))
    assert got == [a, NONE, NONE] and np.isinf(lb3) and np.isinf(carried) and carried > 0
    big = key(np.finfo(F).max, 255)
    assert big < NONE and run([big, big, big])[0] == [big, big, big]


def test_third_bound_is_infinite_exactly_below_three_spheres():
    rng = np.random.default_rng(5)
    for n in range(0, 8):
        keys = [key(s, i) for i, s in enumerate(rng.uniform(0.0, 4.0, n))]
        _, lb3 = run(keys, rf=0.15)
        assert np.isinf(lb3) == (n < 3)
    # negative radius is legal input (sphere.ts just subtracts it); zero distance gives a finite, negative bound
    _, lb3 = run([key(0.0, 0), key(0.0, 1), key(0.0, 2)], rf=0.5)
    assert -0.51 < lb3 < -0.5
    _, lb3 = run([key(1.0, 0), key(1.0, 1), key(1.0, 2)], rf=-0.5)
    assert 1.49 < lb3 < 1.5


def test_the_bound_carried_in_half_a_word_never_exceeds_the_bound():
    """rm_runner_up_pack_bound / _unpack_bound over signs, magnitudes and infinity: the third key's squared distance and the radius
    are chosen so that the bound sweeps positive values from 1e-6 to 1e18 and, with a large radius, negative ones."""
    rng = np.random.default_rng(12)
    seen_pos = seen_neg = 0
    cases = [(10.0 ** rng.uniform(-12, 36), 10.0 ** rng.uniform(-6, 1)) for _ in range(400)]   # (s2, rf): mostly positive bounds
    cases += [(10.0 ** rng.uniform(-6, 2), 10.0 ** rng.uniform(0, 6)) for _ in range(400)]      # large radii: negative bounds
    cases += [(s2, -rf) for s2, rf in cases[:100]]                                              # negative radii
    for s2, rf in cases:
        k = key(s2, 1)
        _, lb3, carried = Context.scan_keys(np.array([k, k, k], np.uint32), rf)
        assert np.isfinite(lb3) and np.isfinite(carried)
        assert carried <= lb3, (s2, rf, lb3, carried)
        if lb3 > 1e-30:
            assert carried >= 0.97 * lb3, (s2, rf, lb3, carried)
            seen_pos += 1
        elif lb3 < -1e-30:
            assert carried >= 1.03 * lb3, (s2, rf, lb3, carried)
            seen_neg += 1
    assert seen_pos >= 300 and seen_neg >= 300
    # the cut keeps seven mantissa bits: the low half of the carried word is zero
    _, _, carried = Context.scan_keys(np.array([key(2.0, 0)] * 3, np.uint32), 0.15)
    assert int(np.array(carried, F).view(np.uint32)) & 0xFFFF == 0
