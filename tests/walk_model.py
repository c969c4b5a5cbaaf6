"""A numpy restatement of how the five marchers walk a ray (rm_ray_walk, include/rm_raymarch.h), as small state machines.
Written from this repository's kernels (csrc/rm_kernels.hip: ray_march, ray_march_other) and oracle; it holds no distance
function and no acceleration structure.  A machine asks for what happens in the next loop trip at parameter t and is told:
the acceleration structure skipped (a SKIP record), a distance was evaluated (an EVAL record), or the acceleration structure
ended the walk.  Two drivers:

  generate(distance, o, d, marcher, ...)  answers every trip with distance(f32(o + d t)): the trace and summary for
                                          acceleration None.
  replay(records, o, d, marcher, ...)     answers every trip with the next record of a given trace and checks that the
                                          record sits at the t the step rule arrived at; when the records run out while
                                          the machine still asks, the acceleration structure ended the walk.

Both derive the summary from the records alone (summarise)."""
import numpy as np

STEP_DTYPE = np.dtype([("t", "<f8"), ("value", "<f8"), ("count", "<u4"), ("kind", "<i4")])
WALK_DTYPE = np.dtype([("t", "<f8"), ("min_dist", "<f8"), ("t_min", "<f8"), ("skipped", "<f8"), ("evals", "<u4"), ("skips", "<u4"),
                       ("sdf_calls", "<u4"), ("end", "<i4")])
EVAL, SKIP = 0, 1
HIT, FAR, STEPS, ACCEL = 0, 1, 2, 3
MAX_DIST, EPSILON = 10.0, 0.001
MARCHERS = ("sphere-tracer", "fixed-step", "adaptive-step", "adaptive-step-v2", "adaptive-step-v3")


def point(o, d, t):
    """f32(o + d t): the binary64 product and sum of the binary32 components, stored to a Float32Array."""
    with np.errstate(all="ignore"):
        return (np.asarray(o, np.float32).astype(np.float64) + np.asarray(d, np.float32).astype(np.float64) * np.float64(t)).astype(np.float32)


def machine(marcher, overshoot=None, step_size=None):
    """Generator over one ray's walk.  Yields ("trip", t): a loop trip at t; send (SKIP, value), (EVAL, value) or None (the
    acceleration structure ended the walk).  AdaptiveStepV3 also yields ("bridge", t): its third evaluation; send the value.
    Returns (t, end) through StopIteration."""
    alg = MARCHERS.index(marcher)
    overshoot = 1.2 if overshoot is None else float(overshoot)
    step_size = 0.1 if step_size is None else float(step_size)
    t = 0.0
    if alg == 0:  # SphereTracer.rayMarch
        for _ in range(100):
            got = yield ("trip", t)
            if got is None:
                return MAX_DIST, ACCEL
            kind, v = got
            t = t + v
            if kind == SKIP:
                if t > MAX_DIST:
                    return t, FAR
                continue
            if v < EPSILON:
                return t, HIT
            if t > MAX_DIST:
                return t, FAR
        return t, STEPS
    fixed = 0.1
    min_step, max_step = fixed * 0.25, fixed * 5.0
    prev_sdf = prev_step = 0.0
    for i in range(200 if alg in (1, 2) else 100):
        got = yield ("trip", t)
        if got is None:
            return MAX_DIST, ACCEL
        kind, v = got
        if kind == SKIP:
            t = t + v
            if t > MAX_DIST:
                return (MAX_DIST if alg in (1, 2) else t), FAR
            prev_sdf = prev_step = 0.0
            continue
        if alg in (1, 2):  # FixedStep, AdaptiveStep: MAX_DIST unless they hit
            if v < EPSILON:
                return t, HIT
            if alg == 1:
                step = step_size
            elif v < 0.1:
                step = 0.01
            else:
                step = 0.8 * v
                if step < min_step:
                    step = min_step
                if step > max_step:
                    step = max_step
            t = t + step
            if t > MAX_DIST:
                return MAX_DIST, FAR
            continue
        # AdaptiveStepV2 / V3
        if v < EPSILON:
            return t, HIT
        if t > MAX_DIST:
            return t, FAR
        if i == 0 or prev_sdf == 0.0:
            t = t + v
            prev_sdf = prev_step = v
            continue
        if prev_step <= prev_sdf + v:  # the spheres overlap: overshoot
            step = v * overshoot
            t = t + step
            prev_sdf, prev_step = v, step
            continue
        if alg == 3:  # step back to the end of the previous sphere
            t = t - prev_step
            t = t + prev_sdf
            prev_step = prev_sdf
            continue
        original = t - prev_step
        t = original + prev_sdf
        d3 = yield ("bridge", t)
        if prev_sdf + v + d3 >= prev_step:
            t = original + prev_step + v
            prev_sdf = prev_step = v
            continue
        prev_sdf = prev_step = d3
        t = t + d3
    return (MAX_DIST if alg in (1, 2) else t), STEPS


def rows_of(records):
    """A trace as a list of (t, value, count, kind) tuples of Python numbers."""
    return records.tolist() if isinstance(records, np.ndarray) else list(records)


def summarise(records, t, end):
    """The rm_walk record of a whole trace, from its records alone."""
    w = np.zeros((), WALK_DTYPE)
    min_dist, t_min, skipped, evals, skips, calls = float("inf"), 0.0, 0.0, 0, 0, 0
    for rt, rv, rc, kind in rows_of(records):
        if kind == EVAL:
            evals += 1
            calls += rc
            if rv < min_dist:
                min_dist, t_min = rv, rt
        else:
            skips += 1
            skipped = skipped + rv
    w["t"], w["min_dist"], w["t_min"], w["skipped"] = t, min_dist, t_min, skipped
    w["evals"], w["skips"], w["sdf_calls"], w["end"] = evals, skips, calls & 0xFFFFFFFF, end
    return w


def generate(distance, o, d, marcher, overshoot=None, step_size=None):
    """The walk of ray (o, d) without an acceleration structure -> (records, summary).  distance(p) -> (value, count) for a
    float32[3] point."""
    m = machine(marcher, overshoot, step_size)
    recs = []
    try:
        what, t = next(m)
        while True:
            v, c = distance(point(o, d, t))
            recs.append((t, float(v), int(c), EVAL))
            what, t = m.send((EVAL, float(v)) if what == "trip" else float(v))
    except StopIteration as e:
        t_end, end = e.value
    records = np.array(recs, STEP_DTYPE)
    return records, summarise(records, t_end, end)


def same(a, b):
    return a == b or (a != a and b != b)


def replay(records, o, d, marcher, overshoot=None, step_size=None):
    """Walks a whole trace: every record must sit at the t the step rule gives from the records before it (after a SKIP:
    t + value), a SKIP must be positive and count nothing, and V3's third evaluation must be an EVAL.  Returns the summary the
    records imply; raises AssertionError at the first record that does not fit.  (o, d) are not needed to follow the rule:
    they are kept in the message.)"""
    m = machine(marcher, overshoot, step_size)
    records = rows_of(records)
    k = 0
    try:
        what, t = next(m)
        while True:
            if k == len(records):
                assert what == "trip", ("the trace ends inside a V3 trip", k, o, d)
                what, t = m.send(None)  # raises StopIteration: the acceleration structure ended the walk
                raise AssertionError("the machine went on after the acceleration structure's end")
            r = records[k]
            rt, rv, rc, kind = r
            assert same(rt, t), ("record %d at t %r, the step rule says %r" % (k, rt, t), o, d)
            k += 1
            if kind == SKIP:
                assert what == "trip" and rv > 0.0 and rc == 0, ("bad SKIP record %d" % (k - 1), r, o, d)
                what, t = m.send((SKIP, rv))
            else:
                assert kind == EVAL, ("unknown record kind", r)
                what, t = m.send((EVAL, rv) if what == "trip" else rv)
    except StopIteration as e:
        t_end, end = e.value
    assert k == len(records), ("%d records after the walk's end" % (len(records) - k), o, d)
    return summarise(records, t_end, end)
