"""Walk queries (rm_ray_walk / rm_ray_walk_device; Context.walk, walk_frame, trace_pixel, Raymarcher.walkBatch): the step
trace and the walk summary of every ray of a batch.  CPU tests: the ABI contract on a host-only context, the numpy model of
tests/walk_model.py against the oracle's renders and against answers derived by hand, and the registers of every walk_kernel
instantiation.  GPU tests: the summaries are rm_ray_march's numbers, every EVAL record is rm_scene_distance at its point,
the model's replay accepts every trace and derives the same summary, the traces under None equal the model driven by the
CPU oracle's distance (and the EVAL values under BVH and Octree the oracle's distances), truncation, the two entries, the
host path's chunks, and a walk query has no side effects."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import walk_model as M  # noqa: E402

ALGS = M.MARCHERS
ACCELS = ("None", "BVH", "Octree")
ANGLE = (0.3, 0.7)
GUARD = 64
FILL = 0xA5
HAND_O = np.array([[0, 0, 3]] * 3, np.float32)
HAND_D = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -1]], np.float32)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def make_query(rm, algorithm="sphere-tracer", time=0.0, overshoot=None, step=None, normal=0):
    N = rm._native
    q = N.rm_ray_query()
    q.algorithm = N.lib().rm_algorithm_from_string(algorithm.encode())
    q.normal = normal  # ignored by a walk query
    q.time = time
    q.overshoot_factor = float("nan") if overshoot is None else overshoot
    q.step_size = float("nan") if step is None else step
    return q


# ----------------------------------------------------------------------------------------------------- CPU: ABI contract

def test_the_library_exports_the_walk_entries_and_the_records_have_their_sizes(rm):
    N = rm._native
    for name in ("rm_ray_walk", "rm_ray_walk_device"):
        assert hasattr(N.lib(), name), name
    assert C.sizeof(N.rm_step) == 24 and C.sizeof(N.rm_walk) == 48
    assert np.dtype(N.STEP_DTYPE) == M.STEP_DTYPE and np.dtype(N.WALK_DTYPE) == M.WALK_DTYPE
    assert M.STEP_DTYPE.itemsize == 24 and M.WALK_DTYPE.itemsize == 48
    assert N.RM_WALK_MAX_STEPS == 256
    assert (N.RM_END_HIT, N.RM_END_FAR, N.RM_END_STEPS, N.RM_END_ACCEL) == (M.HIT, M.FAR, M.STEPS, M.ACCEL)


def test_bad_walk_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    ctx.scene_from_preset(3, 2)
    q = C.byref(make_query(rm))
    o = np.zeros((2, 3), np.float32)
    d = np.ones((2, 3), np.float32)
    w = np.zeros(2, M.WALK_DTYPE)
    s = np.zeros((2, 256), M.STEP_DTYPE)

    def both(q_, n, o_, d_, cap, w_, s_):
        a = L.rm_ray_walk(ctx._h, q_, n, o_, d_, cap, w_, s_)
        b = L.rm_ray_walk_device(ctx._h, q_, n, o_, d_, cap, w_, s_, None)
        assert a == b, (a, b)
        return a

    for n in (2, 0):  # validation comes first, whatever the ray count
        assert both(q, n, vp(o), vp(d), -1, vp(w), vp(s)) == N.RM_E_INVALID
        assert both(q, n, vp(o), vp(d), 257, vp(w), vp(s)) == N.RM_E_INVALID
        assert both(q, n, vp(o), vp(d), -1, vp(w), None) == N.RM_E_INVALID
        assert both(q, n, vp(o), vp(d), 0, vp(w), vp(s)) == N.RM_E_INVALID  # steps given with cap 0
        assert both(q, n, vp(o), vp(d), 0, None, vp(s)) == N.RM_E_INVALID
    assert both(q, 2, vp(o), vp(d), 4, None, None) == N.RM_E_INVALID      # nothing asked for
    assert both(q, 2, vp(o), vp(d), 0, None, None) == N.RM_E_INVALID
    # the device entry: 8-byte alignment of both outputs
    for off in (1, 2, 4):
        assert L.rm_ray_walk_device(ctx._h, q, 2, vp(o), vp(d), 4, C.c_void_p(w.ctypes.data + off), vp(s), None) == N.RM_E_INVALID
        assert L.rm_ray_walk_device(ctx._h, q, 2, vp(o), vp(d), 4, vp(w), C.c_void_p(s.ctypes.data + off), None) == N.RM_E_INVALID
    # rm_ray_march's own checks
    assert both(None, 2, vp(o), vp(d), 4, vp(w), vp(s)) == N.RM_E_INVALID
    assert both(q, -1, vp(o), vp(d), 4, vp(w), vp(s)) == N.RM_E_INVALID
    assert both(q, 2 ** 31, vp(o), vp(d), 4, vp(w), vp(s)) == N.RM_E_INVALID
    assert both(q, 2, None, vp(d), 4, vp(w), vp(s)) == N.RM_E_INVALID
    assert both(q, 2, vp(o), None, 4, vp(w), vp(s)) == N.RM_E_INVALID
    assert L.rm_ray_walk(None, q, 2, vp(o), vp(d), 4, vp(w), vp(s)) == N.RM_E_INVALID
    assert L.rm_ray_walk_device(None, q, 2, vp(o), vp(d), 4, vp(w), vp(s), None) == N.RM_E_INVALID
    # well-formed calls on a host-only context: no device
    assert both(q, 2, vp(o), vp(d), 256, vp(w), vp(s)) == N.RM_E_NO_DEVICE
    assert both(q, 2, vp(o), vp(d), 1, None, vp(s)) == N.RM_E_NO_DEVICE
    assert both(q, 2, vp(o), vp(d), 0, vp(w), None) == N.RM_E_NO_DEVICE
    assert both(q, 2, vp(o), vp(d), 200, vp(w), None) == N.RM_E_NO_DEVICE  # a cap without step records is harmless
    with pytest.raises(rm.RmError) as e:
        ctx.walk(o, d, trace=True)
    assert e.value.code == N.RM_E_NO_DEVICE
    bare = rm.Context(None)  # and the scene check comes last
    assert L.rm_ray_walk(bare._h, q, 2, vp(o), vp(d), -1, vp(w), None) == N.RM_E_INVALID


# ------------------------------------------------------------------------------------------- CPU: the model and the oracle

def oracle_distance(osc, time=0.0):
    return lambda p: osc.distance(p, time)


@pytest.mark.parametrize("alg", ALGS)
def test_the_model_walks_as_the_oracle_renders_without_acceleration(rm, oracle, alg):
    """generate over the 16 x 16 camera rays of preset 2 (nine spheres) against OracleScene.render, pixel for pixel: the depth
    byte is the clamped rounding of t, the iterations are the EVAL records, and the SDF calls are their counts plus getNormal's
    four evaluations of all nine spheres at a hit."""
    W = H = 16
    osc = oracle.OracleScene(preset=2, accel="None")
    osc.set_angles(*ANGLE)
    assert osc.stats()["n"] == 9
    depth, _, sdf, iters = osc.render(W, H, algorithm=alg)
    org, dirs = rm.camera_rays(W, H, *ANGLE)
    ends = set()
    for i in range(W * H):
        recs, w = M.generate(oracle_distance(osc), org, dirs[i], alg)
        t = float(w["t"])
        assert int(min(max(np.rint(t), 0), 255)) == depth[i], (i, t, depth[i])
        assert w["evals"] == len(recs) == iters[i] and w["skips"] == 0 and w["skipped"] == 0.0, (i, w, iters[i])
        assert int(w["sdf_calls"]) + (4 * 9 if t < 10 else 0) == sdf[i], (i, w, sdf[i])
        assert same_bits(M.replay(recs, org, dirs[i], alg), w)
        ends.add(int(w["end"]))
    assert M.HIT in ends and M.ACCEL not in ends and len(ends) >= 2, ends


def test_hand_derived_walks_on_one_sphere(oracle):
    """Preset 0 is one sphere of radius 1.5 at the origin, no acceleration structure."""
    osc = oracle.OracleScene(preset=0, accel="None")
    dist = oracle_distance(osc)
    recs, w = M.generate(dist, HAND_O[0], HAND_D[0], "sphere-tracer")  # towards the sphere
    assert recs.tolist() == [(0.0, 1.5, 1, M.EVAL), (1.5, 0.0, 1, M.EVAL)]
    assert w.tolist() == (1.5, 0.0, 1.5, 0.0, 2, 0, 2, M.HIT)
    recs, w = M.generate(dist, HAND_O[1], HAND_D[1], "sphere-tracer")  # away from it: the distance doubles the step
    assert recs.tolist() == [(0.0, 1.5, 1, M.EVAL), (1.5, 3.0, 1, M.EVAL), (4.5, 6.0, 1, M.EVAL)]
    assert w.tolist() == (10.5, 1.5, 0.0, 0.0, 3, 0, 3, M.FAR)
    recs, w = M.generate(dist, HAND_O[2], HAND_D[2], "fixed-step", step_size=0.005)  # 200 steps of 0.005 end 0.5 short of the surface
    assert len(recs) == 200 and (recs["kind"] == M.EVAL).all() and w["end"] == M.STEPS and w["t"] == 10.0 and w["evals"] == 200
    assert w["t_min"] == recs["t"][199] and w["min_dist"] == recs["value"][199] and abs(w["min_dist"] - 0.505) < 1e-6
    assert abs(recs["t"][199] - 199 * 0.005) < 1e-12
    # replay follows the same rule and refuses a trace that breaks it
    assert same_bits(M.replay(recs, HAND_O[2], HAND_D[2], "fixed-step", step_size=0.005), w)
    bad = recs.copy()
    bad["t"][7] += 1e-9
    with pytest.raises(AssertionError):
        M.replay(bad, HAND_O[2], HAND_D[2], "fixed-step", step_size=0.005)
    with pytest.raises(AssertionError):
        M.replay(recs, HAND_O[2], HAND_D[2], "fixed-step")  # another step size
    # a trace that stops while the marcher would go on is the acceleration structure's end; none at all too
    w = M.replay(recs[:3], HAND_O[2], HAND_D[2], "fixed-step", step_size=0.005)
    assert w["end"] == M.ACCEL and w["t"] == 10.0 and w["evals"] == 3
    w = M.replay(recs[:0], HAND_O[2], HAND_D[2], "sphere-tracer")
    assert w.tolist() == (10.0, float("inf"), 0.0, 0.0, 0, 0, 0, M.ACCEL)
    # skips: the marcher continues at t + value, and the sum is kept
    trace = np.array([(0.0, 0.75, 0, M.SKIP), (0.75, 0.75, 1, M.EVAL), (1.5, 9.0, 0, M.SKIP)], M.STEP_DTYPE)
    w = M.replay(trace, HAND_O[0], HAND_D[0], "sphere-tracer")
    assert w.tolist() == (10.5, 0.75, 0.75, 9.75, 1, 2, 1, M.FAR)
    trace["value"][0] = 0.0
    with pytest.raises(AssertionError):
        M.replay(trace, HAND_O[0], HAND_D[0], "sphere-tracer")


# ------------------------------------------------------------------------------------------------- CPU: build invariants

@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_walk_kernels_spill_nothing(extra):
    """Every walk_kernel<ACCEL, OTHER, GEN>: no VGPR spill; no scratch for spheres and primitive lists (GEN 0 / 1); the
    expression-program interpreter's per-lane scratch (GEN 2 / 3) within the bound of the render and query kernels."""
    from test_build_invariants import HIPCC, assert_no_vgpr_spill, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void walk_kernel<")}
    assert len(kernels) == 24, sorted(kernels)
    assert_no_vgpr_spill(kernels, 800)


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope="module")
def wctx(rm):
    """A context of its own.  Interpreter only: the walk kernels are ahead-of-time, so are the entries they are compared with."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    return c


N_CAM = 64 * 48
I_GOLD, I_HAND, I_MISS, I_INSIDE, I_LONG = N_CAM, N_CAM + 60, N_CAM + 63, N_CAM + 64, N_CAM + 65


@pytest.fixture(scope="module")
def rays(rm, oracle):
    """The 64 x 48 camera rays of ANGLE, the 60 rays of tests/golden/ray_queries.npz, the three hand rays, one ray that
    misses the root box of every preset (it starts beyond it and points away), one that starts at the centre of a sphere of
    preset 3, and two with directions of length 2 and 0.5."""
    org, dirs = rm.camera_rays(64, 48, *ANGLE)
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_queries.npz"))
    centre = oracle.OracleScene(preset=3, accel="None").spheres()[0][0]
    mid = dirs[24 * 64 + 32]
    o = np.concatenate([np.broadcast_to(org, dirs.shape), f["origins"].astype(np.float32).reshape(-1, 3), HAND_O,
                        [[0, 0, 30]], [centre], [org, org]]).astype(np.float32)
    d = np.concatenate([dirs, f["directions"].astype(np.float32).reshape(-1, 3), HAND_D, [[0, 0, 1]], [[0, 1, 0]],
                        [mid * np.float32(2), mid * np.float32(0.5)]]).astype(np.float32)
    assert len(o) == len(d) == I_LONG + 2
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def walk_guarded(rm, ctx, o, d, algorithm="sphere-tracer", time=0.0, overshoot=None, step=None, cap=256, walks=True, steps=True):
    """rm_ray_walk through ctypes, each requested output between two sentinel guards and itself filled with the sentinel ->
    (walks or None, steps[n, cap] or None); the step slots a walk did not reach still hold the sentinel."""
    N = rm._native
    q = make_query(rm, algorithm, time, overshoot, step, normal=1)
    n = len(o)
    raw_w = np.full(n * 48 + 2 * GUARD, FILL, np.uint8) if walks else None
    raw_s = np.full(n * cap * 24 + 2 * GUARD, FILL, np.uint8) if steps else None
    N.check(ctx._h, N.lib().rm_ray_walk(ctx._h, C.byref(q), n, vp(np.ascontiguousarray(o)), vp(np.ascontiguousarray(d)), cap,
                                        C.c_void_p(raw_w.ctypes.data + GUARD) if walks else None,
                                        C.c_void_p(raw_s.ctypes.data + GUARD) if steps else None))
    out = []
    for raw, dt, shape in ((raw_w, M.WALK_DTYPE, (n,)), (raw_s, M.STEP_DTYPE, (n, cap))):
        if raw is None:
            out.append(None)
            continue
        assert (raw[:GUARD] == FILL).all() and (raw[len(raw) - GUARD:] == FILL).all(), "written outside the buffer"
        out.append(np.frombuffer(raw[GUARD:len(raw) - GUARD].tobytes(), dt).reshape(shape))
    return out


def sentinel_behind(steps, length):
    """Every slot past a ray's records still holds the sentinel bytes."""
    n, cap = steps.shape
    mask = np.arange(cap)[None, :] >= np.minimum(length, cap)[:, None]
    return (steps.view(np.uint8).reshape(n, cap, 24)[mask] == FILL).all()


def points_of(o, d, ray, t):
    """f32(o + d t) for records of rays `ray` at parameters t."""
    with np.errstate(all="ignore"):
        return (o[ray].astype(np.float64) + d[ray].astype(np.float64) * t[:, None]).astype(np.float32)


def check(rm, ctx, o, d, what, accel, miss=None, **kw):
    """The equivalence checks (a) - (d) of one scene, marcher and option set -> (walks, steps, lengths)."""
    alg = kw.get("algorithm", "sphere-tracer")
    t, iters, sdf, _ = ctx.ray_march(o, d, alg, normal=False, time=kw.get("time", 0.0), overshoot=kw.get("overshoot"), step=kw.get("step"))
    walks, steps = walk_guarded(rm, ctx, o, d, **kw)
    assert ctx.last_kernel().startswith("walk_kernel<"), ctx.last_kernel()
    # (a) the summary carries rm_ray_march's numbers
    assert same_bits(walks["t"], t) and np.array_equal(walks["evals"], iters) and np.array_equal(walks["sdf_calls"], sdf), what
    length = walks["evals"].astype(np.int64) + walks["skips"]
    assert length.max() <= 200 and sentinel_behind(steps, length), what
    # (b) every EVAL record is Scene.getDistance at f32(o + d t), at the query's time
    live = np.arange(steps.shape[1])[None, :] < length[:, None]
    ev = live & (steps["kind"] == M.EVAL)
    ray, _ = np.nonzero(ev)
    ctx.scene_set_time(kw.get("time", 0.0))
    dist, cnt = ctx.scene_distance(points_of(o, d, ray, steps["t"][ev]))
    assert same_bits(steps["value"][ev], dist) and np.array_equal(steps["count"][ev], cnt), (what, int((steps["value"][ev] != dist).sum()))
    assert set(np.unique(steps["kind"][live]).tolist()) <= {M.EVAL, M.SKIP}
    # (c) the model follows every trace and derives the same summary
    for i in range(len(o)):
        want = M.replay(steps[i, :length[i]], o[i], d[i], alg, kw.get("overshoot"), kw.get("step"))
        assert want.tobytes() == walks[i].tobytes(), (what, i, want, walks[i])
    # (d) skips are positive and count nothing; None never skips and never ends with ACCEL; the root-box miss
    sk = live & (steps["kind"] == M.SKIP)
    assert (steps["value"][sk] > 0).all() and (steps["count"][sk] == 0).all() and sk.sum() == walks["skips"].sum(), what
    if accel == "None":
        assert sk.sum() == 0 and (walks["end"] != M.ACCEL).all() and (walks["skipped"] == 0).all(), what
    if miss is not None:
        assert ctx.scene_info()["root_max"][2] < o[miss][2] and d[miss].tolist() == [0, 0, 1]  # beyond the root box, pointing away
        assert walks[miss].tolist() == (10.0, float("inf"), 0.0, 0.0, 0, 0, 0, M.ACCEL), (what, walks[miss])
    return walks, steps, length


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("accel", ACCELS)
def test_dense_grid_walks_are_the_march_the_distances_and_the_model(rm, wctx, rays, accel, alg):
    rm.Scene(accel, ctx=wctx).loadPreset(3)
    walks, _, _ = check(rm, wctx, *rays, (3, accel, alg), accel, miss=I_MISS if accel == "BVH" else None, algorithm=alg)
    ends = set(walks["end"].tolist())
    assert M.HIT in ends and len(ends) >= 2, ends  # hits and misses both
    if accel != "None":
        assert (walks["skips"] > 0).sum() >= 100 and (walks["skipped"] > 0).sum() >= 100
    print((3, accel, alg), {rm._native.WALK_ENDS[e]: int((walks["end"] == e).sum()) for e in sorted(ends)})


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_marcher_options_reach_the_walk(rm, wctx, rays, accel):
    rm.Scene(accel, ctx=wctx).loadPreset(3)
    o, d = rays
    sel = np.r_[0:N_CAM:7, N_CAM:len(o)]
    check(rm, wctx, o[sel], d[sel], (3, accel, "v2 1.5"), accel, algorithm="adaptive-step-v2", overshoot=1.5)
    check(rm, wctx, o[sel], d[sel], (3, accel, "v3 1.7"), accel, algorithm="adaptive-step-v3", overshoot=1.7)
    walks, _, _ = check(rm, wctx, o[sel], d[sel], (3, accel, "fixed 0.005"), accel, algorithm="fixed-step", step=0.005)
    if accel == "None":
        assert (walks["end"] == M.STEPS).sum() >= 100 and (walks["evals"][walks["end"] == M.STEPS] == 200).all()


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel,time", [(12, "None", 0.7), (12, "BVH", 0.7), (5, "Octree", 0.0), (7, "Octree", 0.0)])
def test_operator_and_primitive_presets(rm, wctx, rays, preset, accel, time):
    rm.Scene(accel, ctx=wctx).loadPreset(preset)
    for alg in ("sphere-tracer", "adaptive-step-v3"):
        check(rm, wctx, *rays, (preset, accel, alg), accel, miss=I_MISS if accel == "BVH" else None, algorithm=alg, time=time)


@pytest.mark.gpu
def test_the_sqrt_length_build(rm, wctx, rays):
    rm.Scene("BVH", ctx=wctx).loadPreset(3)
    wctx.set_option("length", 1)
    try:
        check(rm, wctx, *rays, "length=1", "BVH", miss=I_MISS)
        assert wctx.last_kernel().endswith("[length=sqrt]")
    finally:
        wctx.set_option("length", 0)


@pytest.fixture(scope="module")
def pinned(rays):
    """The 60 golden rays and every 48th camera ray."""
    o, d = rays
    sel = np.r_[I_GOLD:I_GOLD + 60, 0:N_CAM:48]
    return o[sel], d[sel]


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ALGS)
def test_traces_without_acceleration_equal_the_model_on_the_oracles_distance(rm, wctx, oracle, pinned, alg):
    rm.Scene("None", ctx=wctx).loadPreset(3)
    osc = oracle.OracleScene(preset=3, accel="None")
    o, d = pinned
    walks, steps = walk_guarded(rm, wctx, o, d, algorithm=alg)
    for i in range(len(o)):
        recs, w = M.generate(oracle_distance(osc), o[i], d[i], alg)
        assert w.tobytes() == walks[i].tobytes(), (i, w, walks[i])
        assert recs.tobytes() == steps[i, :len(recs)].tobytes(), (i, recs[:3], steps[i, :3])
    assert sentinel_behind(steps, walks["evals"].astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ("BVH", "Octree"))
def test_evaluations_under_acceleration_equal_the_oracles_distance(rm, wctx, oracle, pinned, accel):
    rm.Scene(accel, ctx=wctx).loadPreset(3)
    osc = oracle.OracleScene(preset=3, accel=accel)
    o, d = pinned
    seen = 0
    for alg in ALGS:
        walks, steps = walk_guarded(rm, wctx, o, d, algorithm=alg)
        live = np.arange(steps.shape[1])[None, :] < (walks["evals"].astype(np.int64) + walks["skips"])[:, None]
        ev = live & (steps["kind"] == M.EVAL)
        ray, _ = np.nonzero(ev)
        got = steps[ev]
        want = [osc.distance(p) for p in points_of(o, d, ray, got["t"])]
        assert same_bits(got["value"], np.array([w[0] for w in want], np.float64)), (accel, alg)
        assert np.array_equal(got["count"], np.array([w[1] for w in want], np.uint32)), (accel, alg)
        seen += len(got)
    assert seen >= 1000


@pytest.mark.gpu
def test_truncation_and_absent_outputs(rm, wctx, rays):
    rm.Scene("BVH", ctx=wctx).loadPreset(3)
    o, d = rays
    for alg in ("sphere-tracer", "adaptive-step-v3"):
        walks, steps = walk_guarded(rm, wctx, o, d, algorithm=alg)
        length = walks["evals"].astype(np.int64) + walks["skips"]
        assert (length > 4).sum() >= 100 and (length < 4).sum() >= 1
        w4, s4 = walk_guarded(rm, wctx, o, d, algorithm=alg, cap=4)
        assert same_bits(w4, walks) and sentinel_behind(s4, length)
        keep = np.arange(4)[None, :] < length[:, None]
        assert s4[keep].tobytes() == steps[:, :4][keep].tobytes()
        w1, s1 = walk_guarded(rm, wctx, o, d, algorithm=alg, cap=1)
        assert same_bits(w1, walks) and s1[length > 0].tobytes() == steps[:, :1][length > 0].tobytes()
        w0, none = walk_guarded(rm, wctx, o, d, algorithm=alg, cap=0, steps=False)
        assert none is None and same_bits(w0, walks)
        w0, _ = walk_guarded(rm, wctx, o, d, algorithm=alg, cap=200, steps=False)
        assert same_bits(w0, walks)
        none, s = walk_guarded(rm, wctx, o, d, algorithm=alg, walks=False)
        assert none is None and same_bits(s, steps)


@pytest.mark.gpu
def test_the_device_entry_equals_the_host_entry_on_two_streams(rm, wctx, rays):
    import torch
    N = rm._native
    rm.Scene("Octree", ctx=wctx).loadPreset(3)
    o, d = rays
    kw = (dict(), dict(algorithm="adaptive-step-v3", overshoot=1.5, cap=7))
    want = [wctx.walk(o, d, trace=True, **k) for k in kw]
    for (w, s), k in zip(want, kw):
        gw, gs = walk_guarded(rm, wctx, o, d, algorithm=k.get("algorithm", "sphere-tracer"), overshoot=k.get("overshoot"), cap=k.get("cap", 200))
        length = np.minimum(gw["evals"].astype(np.int64) + gw["skips"], s.shape[1])
        keep = np.arange(s.shape[1])[None, :] < length[:, None]
        assert same_bits(w, gw) and s[keep].tobytes() == gs[keep].tobytes() and not s[~keep].view(np.uint8).any()  # Context.walk zeroes the rest
    to, td = torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for st, k in zip(streams, kw):  # both in flight before either is waited for
        with torch.cuda.stream(st):
            got.append(wctx.walk(to, td, trace=True, **k))
    for st in streams:
        st.synchronize()
    for (gw, gs), (w, s) in zip(got, want):
        assert gw.cpu().numpy().tobytes() == w.tobytes() and gs.cpu().numpy().tobytes() == s.tobytes()
    only = wctx.walk(to, td)  # summaries only
    torch.cuda.synchronize()
    assert only.cpu().numpy().tobytes() == want[0][0].tobytes()
    # no ray: nothing is launched, nothing is written
    q = make_query(rm)
    before = wctx.last_kernel()
    raw = np.full(256, FILL, np.uint8)
    assert N.lib().rm_ray_walk(wctx._h, C.byref(q), 0, vp(np.array(o)), vp(np.array(d)), 4, vp(raw), vp(raw[128:])) == N.RM_OK
    assert N.lib().rm_ray_walk(wctx._h, C.byref(q), 0, None, None, 4, None, None) == N.RM_OK
    guard = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    assert N.lib().rm_ray_walk_device(wctx._h, C.byref(q), 0, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()), 4,
                                      C.c_void_p(guard.data_ptr()), C.c_void_p(guard.data_ptr() + 128), None) == N.RM_OK
    torch.cuda.synchronize()
    assert (raw == FILL).all() and (guard.cpu().numpy() == FILL).all() and wctx.last_kernel() == before
    assert len(wctx.walk(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))) == 0


@pytest.mark.gpu
def test_a_traced_batch_crosses_a_chunk_of_the_host_path(rm, wctx, rays):
    """At cap 256 a chunk of the host path holds 64 MiB / (256 * 24 B) = 10 922 rays: 12 000 rays take two."""
    rm.Scene("BVH", ctx=wctx).loadPreset(3)
    o, d = rays
    n, first = 12000, (64 << 20) // (256 * 24)
    assert first == 10922
    idx = (np.arange(n) * 7) % N_CAM  # camera rays, neighbours unlike each other
    bo, bd = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    walks, steps = walk_guarded(rm, wctx, bo, bd, algorithm="adaptive-step-v2")
    length = walks["evals"].astype(np.int64) + walks["skips"]
    assert sentinel_behind(steps, length)
    for i in (0, first - 1, first, n - 1):
        w1, s1 = walk_guarded(rm, wctx, bo[i:i + 1], bd[i:i + 1], algorithm="adaptive-step-v2")
        assert w1.tobytes() == walks[i:i + 1].tobytes() and s1.tobytes() == steps[i:i + 1].tobytes(), i
    assert same_bits(walk_guarded(rm, wctx, bo, bd, algorithm="adaptive-step-v2", steps=False)[0], walks)


@pytest.mark.gpu
def test_a_walk_query_leaves_armed_diagnostics_and_the_scene_time_alone(rm, wctx, rays):
    import torch
    W, H = 64, 48
    sc = rm.Scene("BVH", ctx=wctx)
    sc.loadPreset(3)
    sc.camera.setAngles(0.2, 0.5)
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    wctx._attach_diag(acc)
    o, d = rays
    wctx.walk(o[:1000], d[:1000], trace=True)
    wctx.walk(torch.from_numpy(np.array(o[:1000])).cuda(), torch.from_numpy(np.array(d[:1000])).cuda(), trace=True)
    wctx.walk_frame(W, H, 0.2, 0.5, device=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "the walk query fired the diagnostics"
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    torch.cuda.synchronize()
    got = wctx.decode_acc(acc)
    s = bufs[2].cpu().numpy().view(np.uint16).astype(np.int64)
    i = bufs[3].cpu().numpy().view(np.uint16).astype(np.int64)
    assert got == {"total_sdf": int(s.sum()), "total_iters": int(i.sum()), "max_sdf": int(s.max()), "min_sdf": int(s.min())}
    sc = rm.Scene("None", ctx=wctx)
    sc.loadPreset(12)
    sc.updateTime(0.5)
    pts = np.array([[0.3, 0.2, -0.1], [1.0, 0.0, 0.0]], np.float32)
    before = wctx.scene_distance(pts)
    wctx.walk(pts, np.ones_like(pts), time=3.25, trace=True)
    after = wctx.scene_distance(pts)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])


@pytest.mark.gpu
def test_the_python_conveniences(rm, wctx):
    sc = rm.Scene("Octree", ctx=wctx)
    sc.loadPreset(3)
    W, H = 40, 24
    org, dirs = rm.camera_rays(W, H, *ANGLE)
    o = np.ascontiguousarray(np.broadcast_to(org, dirs.shape))
    want = wctx.walk(o, dirs, algorithm="adaptive-step")
    frame = wctx.walk_frame(W, H, *ANGLE, algorithm="adaptive-step")
    assert frame.shape == (H, W) and frame.tobytes() == want.tobytes()
    rows = wctx.walk_frame(W, H, *ANGLE, y_start=5, y_end=9, algorithm="adaptive-step")
    assert rows.shape == (4, W) and rows.tobytes() == want[5 * W:9 * W].tobytes()
    dev = wctx.walk_frame(W, H, *ANGLE, algorithm="adaptive-step", device=True)
    assert tuple(dev.shape) == (H, W, 48) and dev.cpu().numpy().tobytes() == want.tobytes()
    got = rm.AdaptiveStepV2(1.5).walkBatch(sc, o, dirs, trace=True, cap=9)
    ref = wctx.walk(o, dirs, algorithm="adaptive-step-v2", overshoot=1.5, trace=True, cap=9)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[1].shape == (W * H, 9)
    w, s = wctx.trace_pixel(W, H, 17, 11, *ANGLE, algorithm="adaptive-step")
    k = 11 * W + 17
    full = wctx.walk(o[k:k + 1], dirs[k:k + 1], algorithm="adaptive-step", trace=True, cap=256)
    assert w.tobytes() == want[k].tobytes() and len(s) == w["evals"] + w["skips"] and s.tobytes() == full[1][0, :len(s)].tobytes()
    # the centre pixel of the one-sphere preset from the default camera is the ray (0, 0, 3) -> (0, 0, -1)
    rm.Scene("None", ctx=wctx).loadPreset(0)
    org, dirs = rm.camera_rays(16, 16, 0.0, 0.0)
    assert org.tolist() == [0, 0, 3] and dirs[8 * 16 + 8].tolist() == [0, 0, -1]
    w, s = wctx.trace_pixel(16, 16, 8, 8)
    assert s.tolist() == [(0.0, 1.5, 1, M.EVAL), (1.5, 0.0, 1, M.EVAL)]
    assert w.tolist() == (1.5, 0.0, 1.5, 0.0, 2, 0, 2, M.HIT)
    ww, ss = walk_guarded(rm, wctx, HAND_O, HAND_D)
    assert ss[1, :3].tolist() == [(0.0, 1.5, 1, M.EVAL), (1.5, 3.0, 1, M.EVAL), (4.5, 6.0, 1, M.EVAL)]
    assert ww[1].tolist() == (10.5, 1.5, 0.0, 0.0, 3, 0, 3, M.FAR)
    ww, ss = walk_guarded(rm, wctx, HAND_O[2:], HAND_D[2:], algorithm="fixed-step", step=0.005)
    assert ww["end"][0] == M.STEPS and ww["t"][0] == 10.0 and ww["evals"][0] == 200 and ww["t_min"][0] == ss["t"][0, 199]
    assert ww["min_dist"][0] == ss["value"][0, 199]
