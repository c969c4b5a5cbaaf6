"""Light queries (rm_ray_light / rm_ray_light_device, rm_phong_light, rm_shade_lit / rm_shade_lit_device; Context.light,
light_frame, shade_lit, phong_light, Raymarcher.lightBatch): shadow rays and ambient occlusion at the hits of a ray query.
CPU tests: the ABI contract on a host-only context, the light direction, the numpy model of tests/light_model.py checked by
hand against the oracle, and the build invariants of every light_kernel instantiation and of shade_lit_kernel.  GPU tests:
every output is bit-identical to the composition of entries pinned elsewhere (rm_ray_march for the primary and the shadow
rays, rm_scene_distance for the occlusion samples, the model for the arithmetic between them), the occlusion term equals one
computed from the CPU oracle alone, the device entry equals the host entry, rm_shade_lit against RM_SHADE_PHONG and the model,
and a light query has no side effects."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import light_model as M  # noqa: E402

ALGS = ("sphere-tracer", "fixed-step", "adaptive-step", "adaptive-step-v2", "adaptive-step-v3")
ACCELS = ("None", "BVH", "Octree")
ANGLE = (0.3, 0.7)
BIAS, K, AO_STEP, AO_STRENGTH = 0.02, 5, 0.05, 1.0  # Context.light's defaults
OUTS = (("t", np.float64, 1), ("iters", np.uint32, 1), ("sdf", np.uint32, 1), ("normal", np.float32, 3), ("lit", np.float32, 1),
        ("ao", np.float32, 1), ("iters2", np.uint32, 1), ("sdf2", np.uint32, 1))
GUARD = 64


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def make_query(rm, algorithm="sphere-tracer", time=0.0, overshoot=None, step=None):
    N = rm._native
    q = N.rm_ray_query()
    q.algorithm = N.lib().rm_algorithm_from_string(algorithm.encode())
    q.normal = 0  # ignored by a light query
    q.time = time
    q.overshoot_factor = float("nan") if overshoot is None else overshoot
    q.step_size = float("nan") if step is None else step
    return q


def make_light(rm, L=None, bias=BIAS, k=K, ao_step=AO_STEP, ao_strength=AO_STRENGTH):
    lt = rm._native.rm_light()
    lt.dir[:] = [float(v) for v in (M.phong_light() if L is None else L)]
    lt.ao_samples, lt.bias, lt.ao_step, lt.ao_strength = k, bias, ao_step, ao_strength
    return lt


# ----------------------------------------------------------------------------------------------------- CPU: ABI contract

def test_the_library_exports_the_light_entries(rm):
    L = rm._native.lib()
    for name in ("rm_ray_light", "rm_ray_light_device", "rm_phong_light", "rm_shade_lit_device", "rm_shade_lit"):
        assert hasattr(L, name), name
    assert C.sizeof(rm._native.rm_light) == 40


def test_phong_light_is_the_models_normalised_direction(rm):
    got = rm.phong_light()
    assert got.dtype == np.float32 and got.tobytes() == M.phong_light().tobytes()
    assert rm._native.lib().rm_phong_light(None) == rm._native.RM_E_INVALID


BAD_LIGHTS = [dict(L=(np.nan, 0, 1)), dict(L=(0, np.inf, 1)), dict(L=(0, 1, -np.inf)), dict(k=-1), dict(k=9), dict(bias=-0.01),
              dict(bias=np.nan), dict(bias=np.inf), dict(ao_strength=-1.0), dict(ao_strength=np.nan), dict(ao_strength=np.inf),
              dict(ao_step=np.nan), dict(ao_step=np.inf), dict(ao_step=0.0), dict(ao_step=-0.05), dict(k=0, ao_step=np.nan)]


def test_bad_light_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    ctx.scene_from_preset(3, 2)
    q = make_query(rm)
    o = np.zeros((2, 3), np.float32)
    d = np.ones((2, 3), np.float32)
    nul = (None,) * 8

    def both(q_, lt_, n, o_, d_):
        a = L.rm_ray_light(ctx._h, q_, lt_, n, o_, d_, *nul)
        b = L.rm_ray_light_device(ctx._h, q_, lt_, n, o_, d_, *nul, None)
        assert a == b, (a, b)
        return a

    good = make_light(rm)
    assert both(C.byref(q), None, 2, vp(o), vp(d)) == N.RM_E_INVALID  # null light
    for bad in BAD_LIGHTS:
        assert both(C.byref(q), C.byref(make_light(rm, **bad)), 2, vp(o), vp(d)) == N.RM_E_INVALID, bad
        assert both(C.byref(q), C.byref(make_light(rm, **bad)), 0, vp(o), vp(d)) == N.RM_E_INVALID, bad  # validation comes first
    # rm_ray_march's own checks
    assert both(None, C.byref(good), 2, vp(o), vp(d)) == N.RM_E_INVALID
    assert both(C.byref(q), C.byref(good), -1, vp(o), vp(d)) == N.RM_E_INVALID
    assert both(C.byref(q), C.byref(good), 2 ** 31, vp(o), vp(d)) == N.RM_E_INVALID
    assert both(C.byref(q), C.byref(good), 2, None, vp(d)) == N.RM_E_INVALID
    assert both(C.byref(q), C.byref(good), 2, vp(o), None) == N.RM_E_INVALID
    assert L.rm_ray_light(None, C.byref(q), C.byref(good), 2, vp(o), vp(d), *nul) == N.RM_E_INVALID
    # well-formed calls on a host-only context: no device (ao_step is free when there are no samples)
    assert both(C.byref(q), C.byref(good), 2, vp(o), vp(d)) == N.RM_E_NO_DEVICE
    assert both(C.byref(q), C.byref(make_light(rm, k=0, ao_step=0.0)), 2, vp(o), vp(d)) == N.RM_E_NO_DEVICE
    assert both(C.byref(q), C.byref(make_light(rm, bias=0.0, ao_strength=0.0)), 2, vp(o), vp(d)) == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.light(o, d)
    assert e.value.code == N.RM_E_NO_DEVICE


def test_bad_shade_lit_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)  # no scene either: the entry never asks for one
    p = np.zeros(256, np.float32)
    a = vp(p)
    odd = C.c_void_p(p.ctypes.data + 2)

    def both(width, rows, n, depth, normal, lit, ao, rgba):
        x = L.rm_shade_lit(ctx._h, width, rows, n, depth, normal, lit, ao, rgba)
        y = L.rm_shade_lit_device(ctx._h, width, rows, n, depth, normal, lit, ao, rgba, None)
        assert x == y, (x, y)
        return x

    for hole in range(5):
        args = [a] * 5
        args[hole] = None
        assert both(4, 4, 1, *args) == N.RM_E_INVALID, hole
    assert both(-1, 4, 1, a, a, a, a, a) == N.RM_E_INVALID
    assert both(4, -1, 1, a, a, a, a, a) == N.RM_E_INVALID
    assert both(4, 4, -1, a, a, a, a, a) == N.RM_E_INVALID
    assert both(4, 4, 65536, a, a, a, a, a) == N.RM_E_INVALID
    assert both(4, 4, 1, a, a, odd, a, a) == N.RM_E_INVALID
    assert both(4, 4, 1, a, a, a, odd, a) == N.RM_E_INVALID
    assert both(4, 4, 1, a, a, a, a, a) == N.RM_E_NO_DEVICE
    assert both(0, 4, 1, a, a, a, a, a) == N.RM_E_NO_DEVICE
    assert L.rm_shade_lit(None, 4, 4, 1, a, a, a, a, a) == N.RM_E_INVALID


# ------------------------------------------------------------------------------------------- CPU: the model, checked by hand

def test_the_model_by_hand_on_one_sphere(oracle):
    """Preset 0 is one sphere of radius 1.5 at the origin: the ray (0, 0, 3) -> (0, 0, -1) hits it at p = (0, 0, 1.5) with
    the normal (0, 0, 1).  A light from behind gives c <= 0: dark, no shadow ray.  The occlusion sum in plain floats."""
    osc = oracle.OracleScene(preset=0, accel="None")
    o = np.array([[0, 0, 3]], np.float32)
    d = np.array([[0, 0, -1]], np.float32)
    t = np.array([1.5])
    nrm = np.array([[0, 0, 1]], np.float32)
    p = M.hit_points(o, d, t)
    assert p.tolist() == [[0.0, 0.0, 1.5]]
    neutral, c, cast = M.classify(t, nrm, (0, 0, -1))
    assert not neutral[0] and c[0] == -1.0 and not cast[0]
    assert M.classify(t, nrm, (0, 0, 1))[2][0]                                      # facing the light: cast
    assert M.classify(np.array([10.0]), nrm, (0, 0, 1))[0][0]                       # a miss is neutral
    assert M.classify(t, np.zeros((1, 3), np.float32), (0, 0, 1))[0][0]             # a zero gradient too
    assert not M.classify(t, np.full((1, 3), np.nan, np.float32), (0, 0, 1))[2][0]  # NaN: not cast
    assert M.shadow_origins(p, nrm, 0.02).tolist() == [[0.0, 0.0, float(np.float32(1.5 + 0.02))]]
    marched = []

    def march(so, sd):
        marched.append(len(so))
        return np.full(len(so), 10.0), np.ones(len(so), np.uint32), np.ones(len(so), np.uint32)

    def distance(pts):
        out = [osc.distance(q) for q in pts]
        return np.array([v[0] for v in out]), np.array([v[1] for v in out], np.uint32)

    step, strength, k_max = 0.05, 2.0, 4
    primary = (t, np.array([7], np.uint32), np.array([11], np.uint32), nrm)
    got = M.compose(o, d, primary, (0, 0, -1), 0.02, k_max, step, strength, march, distance)
    assert not marched and got[4][0] == 0.0 and got[6][0] == 0
    occ, cnt = 0.0, 0
    for k in range(1, k_max + 1):
        q = np.array([0.0, 0.0, np.float32(1.5 + k * step)], np.float32)
        assert M.ao_points(p, nrm, k, step)[0].tobytes() == q.tobytes()
        dk, ck = osc.distance(q)
        assert abs(dk - k * step) < 1e-6  # outside a sphere the distance is the height above it
        occ += (k * step - dk) * 2.0 ** (1 - k)
        cnt += ck
    x = 1.0 - strength * occ
    assert got[5][0] == np.float32(min(max(x, 0.0), 1.0)) and got[7][0] == cnt == k_max
    # a light in front: the shadow ray is cast and its counts lead sdf_calls2
    got = M.compose(o, d, primary, (0, 0, 1), 0.02, k_max, step, strength, march, distance)
    assert marched == [1] and got[4][0] == 1.0 and got[6][0] == 1 and got[7][0] == 1 + k_max
    # the clamp, NaN included
    assert M.ao_value(np.array([[1.0, -1.0, np.nan]]), 0.5, 1.0).tolist() == [1.0, 0.0, 0.0]
    assert M.ao_value(np.zeros((0, 2)), 0.5, 1.0).tolist() == [1.0, 1.0]


def test_the_models_shade_is_the_oracles_phong_within_one_lsb(oracle):
    osc = oracle.OracleScene(preset=3, accel="BVH")
    osc.set_angles(*ANGLE)
    W = H = 48
    dep, nrm, sdf, it = osc.render(W, H)
    want = oracle.shade("phong", dep, nrm, sdf, it, W, H).reshape(-1, 4).astype(np.int16)
    got = M.shade_lit(dep, nrm, np.ones(W * H, np.float32), np.ones(W * H, np.float32)).astype(np.int16)
    assert np.abs(got - want).max() <= 1
    assert (M.shade_lit(dep, nrm, np.ones(W * H, np.float32), np.zeros(W * H, np.float32)) == (0, 0, 0, 255)).all()
    far = M.shade_lit(np.full(2, 255, np.uint8), nrm[:6], np.ones(2, np.float32), np.zeros(2, np.float32))
    assert (far == (10, 10, 20, 255)).all()  # phongModel.ts:38: a depth byte of 255 is the background colour, whatever the terms


# ------------------------------------------------------------------------------------------------- CPU: build invariants

@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_light_kernels_spill_nothing(extra):
    """Every light_kernel<ACCEL, OTHER, GEN>: no VGPR spill; no scratch for spheres and primitive lists (GEN 0 / 1); the
    expression-program interpreter's per-lane scratch (GEN 2 / 3) within the bound of the render and query kernels."""
    from test_build_invariants import HIPCC, assert_no_vgpr_spill, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void light_kernel<")}
    assert len(kernels) == 24, sorted(kernels)
    assert_no_vgpr_spill(kernels, 800)


@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_light_kernels_have_no_spill_ahead_of_an_exec_restore(extra):
    from test_build_invariants import HIPCC, kernel_spans, listing, spill_code_ahead_of_exec_restore
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    lines = listing("rm_kernels.hip", extra)
    spans = kernel_spans(lines, "12light_kernel")
    assert len(spans) == 24, len(spans)
    for a, b in spans:
        assert not spill_code_ahead_of_exec_restore(lines[a:b]), lines[a]


def test_shade_lit_kernel_neither_spills_nor_uses_scratch():
    from test_build_invariants import HIPCC, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    k = [r for n, r in resource_usage((), "rm_frame_ops.hip").items() if n.startswith("shade_lit_kernel(")]
    assert len(k) == 1
    assert k[0]["VGPRs Spill"] == 0 and k[0]["ScratchSize [bytes/lane]"] == 0, k[0]


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope="module")
def lctx(rm):
    """A context of its own.  Interpreter only: the light kernels are ahead-of-time, so are the entries they are compared with."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    return c


@pytest.fixture(scope="module")
def rays(rm):
    """The 64 x 64 camera rays of ANGLE, then the 60 rays of tests/golden/ray_queries.npz."""
    org, dirs = rm.camera_rays(64, 64, *ANGLE)
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ray_queries.npz"))
    o = np.concatenate([np.broadcast_to(org, dirs.shape), f["origins"].astype(np.float32).reshape(-1, 3)])
    d = np.concatenate([dirs, f["directions"].astype(np.float32).reshape(-1, 3)])
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def light_guarded(rm, ctx, o, d, algorithm="sphere-tracer", L=None, bias=BIAS, k=K, ao_step=AO_STEP, ao_strength=AO_STRENGTH, time=0.0,
                  overshoot=None, step=None, only=None):
    """rm_ray_light through ctypes, every requested output between two sentinel guards (the others NULL) -> dict by name."""
    N = rm._native
    q = make_query(rm, algorithm, time, overshoot, step)
    lt = make_light(rm, L, bias, k, ao_step, ao_strength)
    n = len(o)
    raw, ptrs = {}, []
    for name, dt, w in OUTS:
        if only is not None and name not in only:
            ptrs.append(None)
            continue
        raw[name] = np.full(n * w * np.dtype(dt).itemsize + 2 * GUARD, 0xA5, np.uint8)
        ptrs.append(C.c_void_p(raw[name].ctypes.data + GUARD))
    N.check(ctx._h, N.lib().rm_ray_light(ctx._h, C.byref(q), C.byref(lt), n, vp(np.ascontiguousarray(o)), vp(np.ascontiguousarray(d)), *ptrs))
    out = {}
    for name, dt, w in OUTS:
        if name in raw:
            b = raw[name]
            assert (b[:GUARD] == 0xA5).all() and (b[len(b) - GUARD:] == 0xA5).all(), "%s: written outside the buffer" % name
            out[name] = np.frombuffer(b[GUARD:len(b) - GUARD].tobytes(), dt).reshape((n, 3) if w == 3 else (n,))
    return out


def composed(ctx, o, d, algorithm="sphere-tracer", L=None, bias=BIAS, k=K, ao_step=AO_STEP, ao_strength=AO_STRENGTH, time=0.0,
             overshoot=None, step=None):
    """The expectation, from entries pinned elsewhere: rm_ray_march and rm_scene_distance around the model."""
    kw = dict(time=time, overshoot=overshoot, step=step)
    L = M.phong_light() if L is None else np.asarray(L, np.float32)
    primary = ctx.ray_march(o, d, algorithm, normal=True, **kw)
    ctx.scene_set_time(time)
    want = M.compose(o, d, primary, L, bias, k, ao_step, ao_strength,
                     lambda so, sd: ctx.ray_march(so, sd, algorithm, normal=False, **kw)[:3], ctx.scene_distance)
    return dict(zip([name for name, _, _ in OUTS], want))


def assert_equal_outputs(got, want, what):
    for name in got:
        assert same_bits(got[name], want[name]), (what, name, int((got[name] != want[name]).sum()) if got[name].shape == want[name].shape else "shape")


def classes(want, L=None):
    _, _, cast = M.classify(want["t"], want["normal"], M.phong_light() if L is None else L)
    hit = want["t"] < 10
    return dict(miss=int((~hit).sum()), away=int((hit & ~cast).sum()), lit=int((cast & (want["lit"] == 1)).sum()),
                shadowed=int((cast & (want["lit"] == 0)).sum()), occluded=int((want["ao"] < 1).sum()))


def check(rm, ctx, o, d, what, populated=False, **kw):
    want = composed(ctx, o, d, **kw)
    got = light_guarded(rm, ctx, o, d, **kw)
    assert len(o) == 0 or ctx.last_kernel().startswith("light_kernel<"), ctx.last_kernel()  # (no ray: nothing is launched)
    assert_equal_outputs(got, want, what)
    if populated:  # the comparison above says something about every branch of the rule
        cl = classes(want, kw.get("L"))
        print(what, cl)
        assert min(cl.values()) >= 16, (what, cl)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_dense_grid_equals_the_composition_under_every_marcher(rm, lctx, rays, accel):
    rm.Scene(accel, ctx=lctx).loadPreset(3)
    for alg in ALGS:
        check(rm, lctx, *rays, (3, accel, alg), populated=True, algorithm=alg)
    check(rm, lctx, *rays, (3, accel, "options"), populated=True, algorithm="adaptive-step-v2", overshoot=1.5, bias=0.05, k=3, ao_step=0.11,
          ao_strength=2.5)
    check(rm, lctx, *rays, (3, accel, "fixed 0.05"), algorithm="fixed-step", step=0.05, L=(-0.5, 0.25, 2.0), bias=0.0, ao_strength=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel,time", [(12, "None", 0.7), (12, "BVH", 0.7), (5, "Octree", 0.0), (7, "Octree", 0.0)])
def test_operator_and_primitive_presets_equal_the_composition(rm, lctx, rays, preset, accel, time):
    sc = rm.Scene(accel, ctx=lctx)
    sc.loadPreset(preset)
    for alg in ("sphere-tracer", "adaptive-step-v3"):
        check(rm, lctx, *rays, (preset, accel, alg), algorithm=alg, time=time)


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_an_uploaded_primitive_list_equals_the_composition(rm, lctx, oracle, rays, accel):
    sc = rm.Scene(accel, ctx=lctx)
    sc.loadPrims(oracle.OracleScene(accel="None", prims=oracle.synthetic_mixed_prims(40)).prims())
    for alg in ("sphere-tracer", "adaptive-step"):
        check(rm, lctx, *rays, ("mixed 40", accel, alg), algorithm=alg)


@pytest.mark.gpu
def test_the_sqrt_length_build_equals_the_composition(rm, lctx, rays):
    rm.Scene("BVH", ctx=lctx).loadPreset(3)
    lctx.set_option("length", 1)
    try:
        check(rm, lctx, *rays, "length=1", populated=True)
        assert lctx.last_kernel().endswith("[length=sqrt]")
    finally:
        lctx.set_option("length", 0)


@pytest.mark.gpu
def test_ray_counts_sample_counts_and_absent_outputs(rm, lctx, rays):
    rm.Scene("BVH", ctx=lctx).loadPreset(3)
    o, d = rays
    start = 64 * 20  # a row through the grid: hits and misses
    for n in (0, 1, 63, 257):
        for k in (0, 1, 8):
            want = check(rm, lctx, o[start:start + n], d[start:start + n], (n, k), k=k)
            if k == 0:
                assert (want["ao"] == 1).all()
    want = composed(lctx, o[:1000], d[:1000])
    for name, _, _ in OUTS:  # every output absent but one
        got = light_guarded(rm, lctx, o[:1000], d[:1000], only=(name,))
        assert list(got) == [name]
        assert_equal_outputs(got, want, "only " + name)
    assert light_guarded(rm, lctx, o[:1000], d[:1000], only=()) == {}
    # the Python entry and the host mirror give the same arrays
    got = lctx.light(o[:1000], d[:1000])
    assert_equal_outputs(dict(zip([name for name, _, _ in OUTS], got)), want, "Context.light")
    sc = rm.Scene("BVH", ctx=lctx)
    sc.loadPreset(3)
    got = rm.AdaptiveStepV2(1.5).lightBatch(sc, o[:1000], d[:1000], ao_samples=2)
    assert_equal_outputs(dict(zip([name for name, _, _ in OUTS], got)),
                         composed(lctx, o[:1000], d[:1000], algorithm="adaptive-step-v2", overshoot=1.5, k=2), "lightBatch")


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
def test_ambient_occlusion_equals_the_oracles_distances(rm, lctx, oracle, rays, accel):
    """ao and the samples' counts from OracleScene.distance alone, at the model's sample points around the GPU's own hits."""
    rm.Scene(accel, ctx=lctx).loadPreset(3)
    osc = oracle.OracleScene(preset=3, accel=accel)
    o, d = rays
    got = light_guarded(rm, lctx, o, d, L=(0, 0, 0))  # c = 0 everywhere: no shadow ray, sdf2 is the samples' count alone
    idx = np.flatnonzero(~M.classify(got["t"], got["normal"], (0, 0, 0))[0])[::4][:256]
    assert len(idx) == 256
    p = M.hit_points(o[idx], d[idx], got["t"][idx])
    dist = np.zeros((K, 256))
    cnt = np.zeros(256, np.uint32)
    for k in range(1, K + 1):
        for j, q in enumerate(M.ao_points(p, got["normal"][idx], k, AO_STEP)):
            dist[k - 1, j], c = osc.distance(q)
            cnt[j] += c
    want = M.ao_value(dist, AO_STEP, AO_STRENGTH)
    assert same_bits(got["ao"][idx], want), int((got["ao"][idx] != want).sum())
    assert (want < 1).sum() >= 16
    assert np.array_equal(got["sdf2"][idx], cnt) and (got["iters2"] == 0).all() and (got["lit"][idx] == 0).all()


@pytest.mark.gpu
def test_the_device_entry_equals_the_host_entry_on_two_streams(rm, lctx, rays):
    import torch
    rm.Scene("Octree", ctx=lctx).loadPreset(3)
    o, d = rays
    kw = (dict(), dict(algorithm="adaptive-step-v3", ao_samples=8, bias=0.05, light_dir=(0.2, 0.9, 0.4)))
    want = [lctx.light(o, d, **k) for k in kw]
    to, td = torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = []
    for s, k in zip(streams, kw):  # both in flight before either is waited for
        with torch.cuda.stream(s):
            got.append(lctx.light(to, td, **k))
    for s in streams:
        s.synchronize()
    for g, w, k in zip(got, want, kw):
        for a, b, (name, _, _) in zip(g, w, OUTS):
            assert same_bits(a.cpu().numpy(), b), (k, name)
    lit, ao = lctx.light_frame(64, 64, *ANGLE, device=True)
    hl, ha = lctx.light_frame(64, 64, *ANGLE)
    assert same_bits(lit.cpu().numpy(), want[0][4][:4096]) and same_bits(ao.cpu().numpy(), want[0][5][:4096])
    assert same_bits(hl, want[0][4][:4096]) and same_bits(ha, want[0][5][:4096])
    rows = lctx.light_frame(64, 64, *ANGLE, y_start=10, y_end=13)
    assert same_bits(rows[0], want[0][4][640:832]) and same_bits(rows[1], want[0][5][640:832])


@pytest.fixture(scope="module")
def gbuffer(rm, lctx):
    W = H = 64
    sc = rm.Scene("BVH", ctx=lctx)
    sc.loadPreset(3)
    sc.camera.setAngles(*ANGLE)
    bufs = [np.zeros(W * H, np.uint8), np.zeros(3 * W * H, np.uint8), np.zeros(W * H, np.uint16), np.zeros(W * H, np.uint16)]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    for b in bufs:
        b.setflags(write=False)
    assert (bufs[0] < 10).sum() > 500 and (bufs[0] == 10).sum() > 100  # surface and background (the depth byte is round(t))
    return W, H, bufs


@pytest.mark.gpu
def test_shade_lit_is_the_phong_shader_and_the_model(rm, lctx, gbuffer):
    import torch
    W, H, (dep, nrm, sdf, it) = gbuffer
    n = W * H
    dev = [torch.from_numpy(np.array(b).view(np.int16) if b.dtype == np.uint16 else np.array(b)).cuda() for b in (dep, nrm, sdf, it)]
    phong = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    lctx.shade(1, W, H, *dev, phong)  # RM_SHADE_PHONG
    ones = torch.ones(n, dtype=torch.float32, device="cuda")
    out = torch.full((4 * n,), 7, dtype=torch.uint8, device="cuda")
    lctx.shade_lit(dev[0], dev[1], ones, ones, out, W, H)
    assert lctx.last_kernel() == "shade_lit_kernel"
    torch.cuda.synchronize()
    assert torch.equal(out, phong), "lit = ao = 1 is not RM_SHADE_PHONG"

    def host(lit, ao):
        rgba = np.full(4 * n, 7, np.uint8)
        lctx.shade_lit(np.array(dep), np.array(nrm), lit, ao, rgba, W, H)
        return rgba.reshape(-1, 4)

    one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
    assert np.array_equal(host(one, one), phong.cpu().numpy().reshape(-1, 4))
    assert np.array_equal(host(zero, one), M.shade_lit(dep, nrm, zero, one))  # ambient only: no pow
    assert (host(one, zero) == (0, 0, 0, 255)).all()
    rng = np.random.default_rng(5)
    lit, ao = rng.random(n, np.float32), rng.random(n, np.float32)
    diff = np.abs(host(lit, ao).astype(np.int16) - M.shade_lit(dep, nrm, lit, ao).astype(np.int16))
    assert diff.max() <= 1, int(diff.max())


@pytest.mark.gpu
def test_shade_lit_frames_of_one_pixel_and_empty_frames(rm, lctx, gbuffer):
    import torch
    _, _, (dep, nrm, _, _) = gbuffer
    at = np.flatnonzero(dep < 10)[[0, 100, 200]]  # surface pixels
    d3 = np.ascontiguousarray(dep[at])
    n3 = np.ascontiguousarray(nrm.reshape(-1, 3)[at]).reshape(-1)
    lit = np.array([1.0, 0.5, 0.0], np.float32)
    ao = np.array([0.25, 1.0, 1.0], np.float32)
    want = M.shade_lit(d3, n3, lit, ao).astype(np.int16)
    rgba = np.full(12 + 8, 7, np.uint8)
    lctx.shade_lit(d3, n3, lit, ao, rgba[:12], 1, 1, 3)
    assert np.abs(rgba[:12].reshape(3, 4).astype(np.int16) - want).max() <= 1 and (rgba[12:] == 7).all()
    assert np.array_equal(rgba[8:12], want[2].astype(np.uint8))  # (lit = 0: exact)
    t = [torch.from_numpy(a).cuda() for a in (d3, n3, lit, ao)]
    out = torch.full((20,), 7, dtype=torch.uint8, device="cuda")
    lctx.shade_lit(*t, out[:12], 1, 1, 3)
    assert np.array_equal(out.cpu().numpy(), rgba)
    for width, rows, frames in ((0, 5, 3), (5, 0, 3), (1, 1, 0)):
        out.fill_(7)
        lctx.shade_lit(*t, out[:12], width, rows, frames)
        host = np.full(12, 7, np.uint8)
        lctx.shade_lit(d3, n3, lit, ao, host, width, rows, frames)
        assert (out.cpu().numpy() == 7).all() and (host == 7).all(), (width, rows, frames)


@pytest.mark.gpu
def test_a_light_query_leaves_armed_diagnostics_and_the_scene_time_alone(rm, lctx, rays):
    import torch
    W, H = 64, 48
    sc = rm.Scene("BVH", ctx=lctx)
    sc.loadPreset(3)
    sc.camera.setAngles(0.2, 0.5)
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    lctx._attach_diag(acc)
    o, d = rays
    lctx.light(o[:1000], d[:1000])
    lctx.light(torch.from_numpy(np.array(o[:1000])).cuda(), torch.from_numpy(np.array(d[:1000])).cuda())
    lctx.light_frame(W, H, 0.2, 0.5, device=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "the light query fired the diagnostics"
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    torch.cuda.synchronize()
    got = lctx.decode_acc(acc)
    s = bufs[2].cpu().numpy().view(np.uint16).astype(np.int64)
    i = bufs[3].cpu().numpy().view(np.uint16).astype(np.int64)
    assert got == {"total_sdf": int(s.sum()), "total_iters": int(i.sum()), "max_sdf": int(s.max()), "min_sdf": int(s.min())}
    sc = rm.Scene("None", ctx=lctx)
    sc.loadPreset(12)
    sc.updateTime(0.5)
    pts = np.array([[0.3, 0.2, -0.1], [1.0, 0.0, 0.0]], np.float32)
    before = lctx.scene_distance(pts)
    lctx.light(pts, np.ones_like(pts), time=3.25)
    after = lctx.scene_distance(pts)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
