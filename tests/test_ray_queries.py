"""Ray queries (rm_ray_march / rm_ray_march_device / rm_camera_rays; Context.ray_march, camera_rays, the host mirror's
Raymarcher.rayMarch / getNormal / rayMarchBatch): Raymarcher.rayMarch (+ getNormal) of the reference for rays of any origin
and direction.  CPU tests: the ABI contract on a host-only context, camera_rays against a numpy restatement of
raymarcher.ts:73,83-88, and the build invariants of every cast_kernel instantiation.  GPU tests: the rays of camera_rays
reproduce the oracle's runRaymarcher pixel for pixel, the device entry equals the host entry, knobs change no bit, a ray
query leaves armed render diagnostics alone, and the host mirror called pixel by pixel reproduces runRaymarcher."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ACCELS = ("None", "Octree", "BVH")
ALGS = ("sphere-tracer", "fixed-step", "adaptive-step", "adaptive-step-v2", "adaptive-step-v3")
ANGLES = ((0.0, 0.0), (0.3, 0.7), (-1.2, 2.5))


def u8clamp(x):
    """Uint8ClampedArray store: round half to even, clamp to [0, 255], NaN -> 0."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 0.0, np.clip(np.rint(x), 0, 255)).astype(np.uint8)


def quantise_normal(n):
    return u8clamp((np.asarray(n, np.float32).astype(np.float64) + 1) * 0.5 * 255).reshape(-1)


# ----------------------------------------------------------------------------------------------------- CPU: ABI contract

def test_host_only_context_refuses_to_march(rm):
    ctx = rm.Context(None)
    with pytest.raises(rm.RmError) as e:
        ctx.ray_march(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    assert e.value.code == rm._native.RM_E_NO_DEVICE


def test_bad_arguments_are_invalid(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    q = N.rm_ray_query()
    o = np.zeros((2, 3), np.float32)
    d = np.ones((2, 3), np.float32)
    out = np.zeros(8, np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.rm_ray_march(ctx._h, None, 2, vp(o), vp(d), None, None, None, None) == N.RM_E_INVALID  # null query
    assert L.rm_ray_march(ctx._h, C.byref(q), -1, vp(o), vp(d), vp(out), None, None, None) == N.RM_E_INVALID
    assert L.rm_ray_march(ctx._h, C.byref(q), 2, None, vp(d), vp(out), None, None, None) == N.RM_E_INVALID
    assert L.rm_ray_march(ctx._h, C.byref(q), 2, vp(o), None, vp(out), None, None, None) == N.RM_E_INVALID
    assert L.rm_ray_march(ctx._h, C.byref(q), 2 ** 31, vp(o), vp(d), vp(out), None, None, None) == N.RM_E_INVALID
    assert L.rm_ray_march(None, C.byref(q), 2, vp(o), vp(d), vp(out), None, None, None) == N.RM_E_INVALID
    assert L.rm_ray_march_device(ctx._h, None, 2, vp(o), vp(d), None, None, None, None, None) == N.RM_E_INVALID
    assert L.rm_ray_march_device(ctx._h, C.byref(q), -5, vp(o), vp(d), None, None, None, None, None) == N.RM_E_INVALID
    assert L.rm_ray_march_device(ctx._h, C.byref(q), 2, None, None, None, None, None, None, None) == N.RM_E_INVALID
    # well-formed arguments on a host-only context: no device
    assert L.rm_ray_march(ctx._h, C.byref(q), 2, vp(o), vp(d), vp(out), None, None, None) == N.RM_E_NO_DEVICE
    assert L.rm_ray_march_device(ctx._h, C.byref(q), 2, vp(o), vp(d), None, None, None, None, None) == N.RM_E_NO_DEVICE


def test_unknown_algorithm_names_are_the_sphere_tracer(rm):
    L = rm._native.lib()
    for name in (b"nonsense", b"", b"Sphere-Tracer", None):
        assert L.rm_algorithm_from_string(name) == 0
    for i, name in enumerate(ALGS):
        assert L.rm_algorithm_from_string(name.encode()) == i


# ------------------------------------------------------------------------------------------------- CPU: camera_rays

def numpy_camera_rays(oracle, W, H, pitch, yaw, y0, y1):
    """raymarcher.ts:73,83-88 restated on the oracle's camera: vec3.fromValues (f32), transformMat3 (f32), normalize (f32)."""
    sc = oracle.OracleScene(preset=0, accel="None")
    sc.set_angles(pitch, yaw)
    rot, org = sc.camera()
    r = rot.astype(np.float64)
    ys, xs = np.meshgrid(np.arange(y0, y1, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    v = (ys / H - 0.5) * 2.0
    u = (xs / W - 0.5) * 2.0
    ax = u.astype(np.float32).astype(np.float64)
    ay = v.astype(np.float32).astype(np.float64)
    az = -1.0
    dx = (ax * r[0] + ay * r[3] + az * r[6]).astype(np.float32).astype(np.float64)
    dy = (ax * r[1] + ay * r[4] + az * r[7]).astype(np.float32).astype(np.float64)
    dz = (ax * r[2] + ay * r[5] + az * r[8]).astype(np.float32).astype(np.float64)
    ln = dx * dx + dy * dy + dz * dz
    ln = np.where(ln > 0, 1 / np.sqrt(np.where(ln > 0, ln, 1.0)), ln)
    d = np.stack([dx * ln, dy * ln, dz * ln], axis=-1).astype(np.float32).reshape(-1, 3)
    return org, d


@pytest.mark.parametrize("W,H", [(64, 48), (97, 61), (33, 17)])
@pytest.mark.parametrize("ang", [(0.0, 0.0), (0.3, 0.7), (math.pi / 2, 1.0), (-math.pi / 2, -0.4)])
def test_camera_rays_restate_runraymarcher(rm, oracle, W, H, ang):
    org, dirs = rm.camera_rays(W, H, *ang)
    want_org, want = numpy_camera_rays(oracle, W, H, *ang, 0, H)
    assert org.tobytes() == want_org.tobytes()
    assert dirs.shape == (W * H, 3) and dirs.tobytes() == want.tobytes()
    _, org2 = rm.camera_from_angles(*ang)
    assert org.tobytes() == org2.tobytes()
    # a row subset is the same rows of the full frame
    y0, y1 = H // 3, H // 3 + 7
    org3, sub = rm.camera_rays(W, H, *ang, y_start=y0, y_end=y1)
    assert org3.tobytes() == org.tobytes() and sub.tobytes() == dirs[y0 * W:y1 * W].tobytes()


def test_camera_rays_rejects_bad_frames(rm):
    for args in [(0, 0, 0.0, 0.0), (4, 4, float("nan"), 0.0), (4, 4, 0.0, float("inf"))]:
        with pytest.raises(rm.RmError):
            rm.camera_rays(*args)
    with pytest.raises(rm.RmError):
        rm.camera_rays(4, 4, 0.0, 0.0, y_start=3, y_end=5)
    org, d = rm.camera_rays(0, 4, 0.0, 0.0)
    assert d.shape == (0, 3) and np.isfinite(org).all()


# ------------------------------------------------------------------------------------------------- CPU: build invariants

@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_cast_kernels_spill_nothing(extra):
    from test_build_invariants import HIPCC, assert_no_vgpr_spill, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void cast_kernel<")}
    assert len(kernels) == 24, sorted(kernels)
    assert_no_vgpr_spill(kernels)


@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_cast_kernels_have_no_spill_ahead_of_an_exec_restore(extra):
    from test_build_invariants import HIPCC, kernel_spans, listing, spill_code_ahead_of_exec_restore
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    lines = listing("rm_kernels.hip", extra)
    spans = kernel_spans(lines, "11cast_kernel")
    assert len(spans) == 24, len(spans)
    for a, b in spans:
        assert not spill_code_ahead_of_exec_restore(lines[a:b]), lines[a]


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope="module")
def rctx(rm):
    """A context of its own: options set here never leak into other test modules."""
    return rm.Context(0)


def _scene(rm, ctx, preset, accel):
    sc = rm.Scene(accel, ctx=ctx)
    sc.loadPreset(preset)
    return sc


def _march_frame(rm, ctx, preset, accel, W, H, ang, rows, alg, time=0.0, overshoot=None, step=None):
    y0, y1 = rows
    _scene(rm, ctx, preset, accel)
    org, dirs = rm.camera_rays(W, H, *ang, y_start=y0, y_end=y1)
    o = np.broadcast_to(org, dirs.shape).copy()
    return ctx.ray_march(o, dirs, alg, normal=True, time=time, overshoot=overshoot, step=step)


def _assert_frame(got, want, what):
    t, it, sdf, nrm = got
    depth, normal, s16, i16 = want
    assert np.array_equal(u8clamp(t), depth), what + ": depth"
    assert np.array_equal(quantise_normal(nrm), normal), what + ": normal"
    assert np.array_equal((sdf & 0xFFFF).astype(np.uint16), s16), what + ": sdf"
    assert np.array_equal((it & 0xFFFF).astype(np.uint16), i16), what + ": iters"


PRESETS = (0, 2, 3, 5, 9, 10, 13, 15, 17)


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("preset", PRESETS)
def test_camera_rays_reproduce_the_oracle(rm, oracle, rctx, preset, accel):
    """Every marcher at every angle on a 64 x 48 frame, and a row tile of 97 x 61."""
    sc = oracle.OracleScene(preset=preset, accel=accel)
    cases = [(64, 48, ang, (0, 48), alg) for alg in ALGS for ang in ANGLES]
    cases += [(97, 61, (-1.2, 2.5), (17, 40), alg) for alg in ("sphere-tracer", "adaptive-step-v3")]
    for W, H, ang, rows, alg in cases:
        sc.set_angles(*ang)
        want = sc.render(W, H, rows[0], rows[1], algorithm=alg)
        got = _march_frame(rm, rctx, preset, accel, W, H, ang, rows, alg)
        _assert_frame(got, want, "preset %d %s %s %s %dx%d" % (preset, accel, alg, ang, W, H))
        assert rctx.last_kernel().startswith("cast_kernel<")


@pytest.mark.gpu
@pytest.mark.parametrize("specialise", [0, 1])
@pytest.mark.parametrize("length", [0, 1])
def test_camera_rays_equal_runraymarcher_in_both_length_modes(rm, oracle, rctx, length, specialise):
    """The library's own render of the same frame (its kernel choice under `specialise`, forests included) and the oracle,
    in both vec3.length modes, for all five marchers."""
    W, H, ang = 64, 48, (0.3, 0.7)
    rctx.set_option("specialise", specialise)
    rctx.set_option("length", length)
    oracle.lib().ro_set_length_mode(length)
    try:
        for preset, accel in [(3, "BVH"), (3, "Octree"), (2, "None"), (9, "BVH"), (15, "Octree"), (17, "None")]:
            ref = oracle.OracleScene(preset=preset, accel=accel)
            ref.set_angles(*ang)
            for alg in ALGS:
                sc = _scene(rm, rctx, preset, accel)
                sc.camera.setAngles(*ang)
                bufs = (np.zeros(W * H, np.uint8), np.zeros(3 * W * H, np.uint8), np.zeros(W * H, np.uint16), np.zeros(W * H, np.uint16))
                rm.createRaymarcher(alg).runRaymarcher(sc, *bufs, W, H, 0.0)
                got = _march_frame(rm, rctx, preset, accel, W, H, ang, (0, H), alg)
                what = "preset %d %s %s length=%d specialise=%d" % (preset, accel, alg, length, specialise)
                _assert_frame(got, bufs, what + " vs runRaymarcher")
                _assert_frame(got, ref.render(W, H, algorithm=alg), what + " vs oracle")
    finally:
        rctx.set_option("length", 0)
        rctx.set_option("specialise", 1)
        oracle.lib().ro_set_length_mode(0)


@pytest.mark.gpu
def test_animated_preset_takes_the_query_time(rm, oracle, rctx):
    W, H, ang = 64, 48, (0.3, 0.7)
    sc = oracle.OracleScene(preset=12, accel="BVH")
    sc.set_angles(*ang)
    for time in (0.0, 1.75):
        got = _march_frame(rm, rctx, 12, "BVH", W, H, ang, (0, H), "sphere-tracer", time=time)
        _assert_frame(got, sc.render(W, H, time=time), "preset 12 time %g" % time)


@pytest.mark.gpu
def test_step_options_reach_the_marchers(rm, oracle, rctx):
    W, H, ang = 64, 48, (0.3, 0.7)
    sc = oracle.OracleScene(preset=3, accel="BVH")
    sc.set_angles(*ang)
    for alg, ov, st in [("fixed-step", None, 0.05), ("adaptive-step-v2", 1.5, None), ("adaptive-step-v3", 1.1, None)]:
        got = _march_frame(rm, rctx, 3, "BVH", W, H, ang, (0, H), alg, overshoot=ov, step=st)
        _assert_frame(got, sc.render(W, H, algorithm=alg, overshoot_factor=ov, step_size=st), alg)
    # an unknown rm_algorithm value is the sphere tracer (raymarchWorker.ts:49-68)
    o, d = rm.camera_rays(W, H, *ang)
    o = np.broadcast_to(o, d.shape).copy()
    a = rctx.ray_march(o, d, 0)
    b = rctx.ray_march(o, d, 99)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def random_rays(n, seed=5):
    """Origins all over (inside the octree cube, outside it, on the camera orbit), directions unnormalised, some with
    exact-zero components."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-12, 12, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32) * rng.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    d[::7, 0] = 0
    d[::11, 1] = 0
    d[::13, 2] = 0
    d[::29] = [0, 0, -1]
    o[::3] = o[::3] * np.float32(0.25)
    return o, d


@pytest.mark.gpu
def test_device_entry_equals_host_entry(rm, rctx):
    import torch
    _scene(rm, rctx, 3, "BVH")
    s = torch.cuda.Stream()
    for n in (1, 255, 257, 5000):
        o, d = random_rays(n, seed=n)
        want = rctx.ray_march(o, d, "adaptive-step-v3" if n == 257 else "sphere-tracer")
        with torch.cuda.stream(s):
            got = rctx.ray_march(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(),
                                 "adaptive-step-v3" if n == 257 else "sphere-tracer")
        s.synchronize()
        for g, w, name in zip(got, want, ("t", "iters", "sdf", "normal")):
            g = g.cpu().numpy()
            assert g.view(np.uint8).tobytes() == np.ascontiguousarray(w).view(np.uint8).tobytes(), (n, name)


@pytest.mark.gpu
def test_a_large_batch_equals_the_same_rays_in_chunks(rm, rctx):
    import torch
    _scene(rm, rctx, 3, "Octree")
    n = 3 * 1024 * 1024 + 77
    o, d = random_rays(n, seed=3)
    og, dg = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    whole = rctx.ray_march(og, dg)
    cuts = np.linspace(0, n, 8).astype(int)
    parts = [rctx.ray_march(og[a:b].contiguous(), dg[a:b].contiguous()) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in range(4):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    # and the host entry, which goes through the scratch buffer in chunks of its own
    sel = slice(0, 1 << 20)
    host = rctx.ray_march(o[sel], d[sel])
    assert np.array_equal(host[0], whole[0][sel].cpu().numpy()) and np.array_equal(host[2], whole[2][sel].cpu().numpy().view(np.uint32))


@pytest.mark.gpu
def test_without_normals_only_the_four_getnormal_evaluations_go(rm, rctx):
    """On a one-primitive scene without acceleration every Scene.getDistance counts 1: getNormal adds exactly 4 per hit."""
    for preset, accel in [(0, "None"), (5, "None")]:
        _scene(rm, rctx, preset, accel)
        o, d = random_rays(20000, seed=preset + 1)
        t1, i1, s1, n1 = rctx.ray_march(o, d, normal=True)
        t0, i0, s0, n0 = rctx.ray_march(o, d, normal=False)
        hit = ~(t1 >= 10)
        assert hit.any() and (~hit).any()
        assert np.array_equal(t0.view(np.uint64), t1.view(np.uint64)) and np.array_equal(i0, i1)
        assert np.array_equal(s1 - s0, np.where(hit, 4, 0).astype(np.uint32))
        assert not n0.any() and not n1[~hit].any()
        assert np.allclose(np.linalg.norm(n1[hit], axis=1), 1, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel", [(3, "BVH"), (3, "Octree"), (2, "BVH"), (3, "None")])
def test_knobs_change_no_bit(rm, rctx, preset, accel):
    _scene(rm, rctx, preset, accel)
    o, d = random_rays(30000, seed=9)
    co, cd = rm.camera_rays(80, 60, 0.3, 0.7)
    o = np.concatenate([o, np.broadcast_to(co, cd.shape)])
    d = np.concatenate([d, cd])
    base = rctx.ray_march(o, d)
    for key in ("filter", "v1_lists", "grid", "lut", "recs", "sub"):
        old = rctx.get_option(key)
        for v in (0, 1):
            rctx.set_option(key, v)
            _scene(rm, rctx, preset, accel)
            got = rctx.ray_march(o, d)
            assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(got, base)), (key, v)
        rctx.set_option(key, old)


@pytest.mark.gpu
def test_a_ray_query_leaves_armed_diagnostics_to_the_render(rm, rctx):
    import torch
    W, H = 64, 48
    sc = _scene(rm, rctx, 3, "BVH")
    sc.camera.setAngles(0.2, 0.5)
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    rctx._attach_diag(acc)
    o, d = random_rays(1000)
    rctx.ray_march(o, d)  # host entry
    rctx.ray_march(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())  # device entry
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "the ray query fired the diagnostics"
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    torch.cuda.synchronize()
    got = rctx.decode_acc(acc)
    s = bufs[2].cpu().numpy().view(np.uint16).astype(np.int64)
    i = bufs[3].cpu().numpy().view(np.uint16).astype(np.int64)
    assert got == {"total_sdf": int(s.sum()), "total_iters": int(i.sum()), "max_sdf": int(s.max()), "min_sdf": int(s.min())}


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel,alg", [(3, "BVH", "sphere-tracer"), (2, "Octree", "adaptive-step-v2"), (9, "None", "fixed-step")])
def test_host_mirror_pixel_by_pixel_is_runraymarcher(rm, rctx, preset, accel, alg):
    W = H = 16
    ang = (0.3, 0.7)
    sc = _scene(rm, rctx, preset, accel)
    sc.camera.setAngles(*ang)
    march = rm.createRaymarcher(alg)
    want = (np.zeros(W * H, np.uint8), np.zeros(3 * W * H, np.uint8), np.zeros(W * H, np.uint16), np.zeros(W * H, np.uint16))
    march.runRaymarcher(sc, *want, W, H, 0.0)
    org, dirs = rm.camera_rays(W, H, *ang)
    depth, normal = np.zeros(W * H, np.uint8), np.zeros(3 * W * H, np.uint8)
    sdf, iters = np.zeros(W * H, np.uint16), np.zeros(W * H, np.uint16)
    for idx in range(W * H):  # raymarcher.ts:76-108
        t = march.rayMarch(sc, org, dirs[idx], idx, sdf, iters)
        hitp = (org.astype(np.float64) + dirs[idx].astype(np.float64) * t).astype(np.float32)  # vec3.scaleAndAdd
        n = np.zeros(3, np.float32) if t >= march.getMaxDistance() else march.getNormal(sc, hitp, idx, sdf)
        normal[3 * idx:3 * idx + 3] = quantise_normal(n)
        depth[idx] = u8clamp(t)
    for got, w, name in zip((depth, normal, sdf, iters), want, ("depth", "normal", "sdf", "iters")):
        assert np.array_equal(got, w), name
    t, it, s, nb = march.rayMarchBatch(sc, np.broadcast_to(org, dirs.shape), dirs)
    assert np.array_equal(u8clamp(t), want[0]) and np.array_equal(quantise_normal(nb), want[1])
    assert np.array_equal((s & 0xFFFF).astype(np.uint16), want[2]) and np.array_equal((it & 0xFFFF).astype(np.uint16), want[3])


# --------------------------------------------- the reference's own rayMarch / getNormal for arbitrary rays (recorded fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_FIXTURE = os.path.join(ROOT, "tests", "golden", "ray_queries.npz")


def _crosscheck():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import ray_crosscheck
    return ray_crosscheck


def _fixture():
    import json
    f = dict(np.load(RAY_FIXTURE))
    return f, json.loads(str(f["configs"]))


def test_ray_fixture_covers_every_category_and_configuration(rm):
    X = _crosscheck()
    assert os.path.getsize(RAY_FIXTURE) < 256 * 1024
    f, cfgs = _fixture()
    o, d, cat = X.ray_set()
    assert f["origins"].tobytes() == o.tobytes() and f["directions"].tobytes() == d.tobytes() and f["category"].tobytes() == cat.tobytes()
    C, N = len(cfgs), len(o)
    assert f["t_bits"].shape == (C, N) and f["sdf"].shape == (C, N) and f["iters"].shape == (C, N)
    assert f["normal_bits"].shape == (C, N, 3) and f["inside"].shape == (C, N)
    # configurations, stated independently of the recorder
    have = {(c.get("preset"), c["accel"], c["algorithm"]) for c in cfgs}
    for p in range(19):
        if p != 13:
            assert all((p, a, "sphere-tracer") in have for a in ACCELS), p
    for p in (0, 2, 3, 5, 17):
        assert all((p, a, alg) in have for a in ACCELS for alg in ALGS), p
    assert any(c["algorithm"] == "fixed-step" and c.get("stepSize") not in (None, 0.1) for c in cfgs)
    for alg in ("adaptive-step-v2", "adaptive-step-v3"):
        assert any(c["algorithm"] == alg and c.get("overshootFactor") not in (None, 1.2) for c in cfgs), alg
    assert any(c.get("preset") == 12 and c.get("time", 0) != 0 for c in cfgs)
    assert any(c.get("synthetic") == 1000 and c["accel"] == "Octree" for c in cfgs)
    assert not any(c.get("preset") == 13 for c in cfgs)  # node's Math.pow is not fdlibm's (README)
    # ray categories
    names = [str(n) for n in f["category_names"]]
    assert names == ["orbit", "in_root_box", "in_primitive", "outside_cube", "zero_components", "unnormalised", "away"]
    sel = {n: cat == k for k, n in enumerate(names)}
    assert all(m.any() for m in sel.values())
    assert np.allclose(np.linalg.norm(o[sel["orbit"]], axis=1), 3, atol=1e-5)
    assert (np.abs(o[sel["outside_cube"]]).max(axis=1) > 10).all() and (np.abs(o[sel["away"]]).max(axis=1) > 10).all()
    assert (d[sel["zero_components"]] == 0).any(axis=1).all()
    assert (np.abs(np.linalg.norm(d[sel["unnormalised"]], axis=1) - 1) > 1e-3).all()
    t = f["t_bits"].view(np.float64)
    finite_scene = [k for k, c in enumerate(cfgs) if c.get("preset") != 15]  # preset 15 repeats its object without end
    assert (t[np.ix_(finite_scene, np.where(sel["away"])[0])] >= 10).all()
    inside = f["inside"].astype(bool)
    for k, c in enumerate(cfgs):  # the one-sphere preset: every in_primitive origin is inside (reference's Scene.getDistance < 0)
        if c.get("preset") == 0:
            assert inside[k, sel["in_primitive"]].all(), c
    assert inside[:, sel["in_primitive"]].any(axis=1).mean() > 0.5
    ctx = rm.Context(None)  # host-only: scene building only
    for p in range(19):
        if p == 13:
            continue
        ctx.scene_from_preset(p, 2)
        info = ctx.scene_info()
        lo, hi = np.array(info["root_min"], np.float32), np.array(info["root_max"], np.float32)
        ob = o[sel["in_root_box"]]
        assert ((ob >= lo) & (ob <= hi)).all(axis=1).any(), p


def test_ray_fixture_regenerates_byte_for_byte(tmp_path):
    X = _crosscheck()
    if not X.available():
        pytest.skip("node or the reference sources not present (scripts/ray_crosscheck.py runs on the build machine only)")
    out = str(tmp_path / "ray_queries.npz")
    X.record(out)
    assert open(out, "rb").read() == open(RAY_FIXTURE, "rb").read()


@pytest.mark.gpu
def test_arbitrary_rays_reproduce_the_reference_flow(rm, rctx):
    """Every configuration of the fixture, bit for bit: rayMarch's f64 result, getNormal's f32 normal, the counters mod 65536."""
    from cpu_raymarcher_amd.synthetic import synthetic_spheres
    f, cfgs = _fixture()
    o, d, cat = f["origins"], f["directions"], f["category"]
    names = [str(n) for n in f["category_names"]]
    bad = []
    for k, cfg in enumerate(cfgs):
        sc = rm.Scene(cfg["accel"], ctx=rctx)
        if "synthetic" in cfg:
            sp = synthetic_spheres(cfg["synthetic"])
            sc.loadSpheres(sp[:, :3], sp[:, 3])
        else:
            sc.loadPreset(cfg["preset"])
        t, it, s, n = rctx.ray_march(o, d, cfg["algorithm"], normal=True, time=cfg.get("time", 0.0),
                                     overshoot=cfg.get("overshootFactor"), step=cfg.get("stepSize"))
        wrong = (t.view(np.uint64) != f["t_bits"][k]) | (n.view(np.uint32) != f["normal_bits"][k]).any(axis=1)
        wrong |= ((s & 0xFFFF).astype(np.uint16) != f["sdf"][k]) | ((it & 0xFFFF).astype(np.uint16) != f["iters"][k])
        if wrong.any():
            bad.append((cfg, sorted({names[c] for c in cat[wrong]}), int(wrong.sum())))
    assert not bad, bad[:6]


@pytest.mark.gpu
def test_a_ray_query_leaves_the_scene_time_alone(rm, rctx):
    sc = _scene(rm, rctx, 12, "None")
    sc.updateTime(0.5)
    pts = np.array([[0.3, 0.2, -0.1], [1.0, 0.0, 0.0]], np.float32)
    before = rctx.scene_distance(pts)
    rctx.ray_march(pts, np.ones_like(pts), time=3.25)
    after = rctx.scene_distance(pts)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
