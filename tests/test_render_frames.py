"""rm_render_frames_device / Context.render_frames: n frames of one scene in one launch, and rm_sweep_views.

Every expectation comes from the CPU oracle -- OracleScene.set_angles + .render for the G-buffers, oracle.shade for rgba,
oracle.diagnostics for the accumulators -- never from the library's own single-frame render.  Bar as everywhere in the
project: G-buffers and counters bit-exact, rgba bit-exact except Phong (1 LSB per channel: Math.pow).  The job's own camera
and time are set to values no view uses: the entry must ignore them."""
import ctypes as C
import math

import numpy as np
import pytest

NAMES = ("depth", "normal", "sdf", "iters")
NEUTRAL = {"total_sdf": 0, "total_iters": 0, "max_sdf": 0, "min_sdf": 0xFFFFFFFF}
ACCEL = {"None": 0, "Octree": 1, "BVH": 2}
SENTINEL = 0xA5
# pitch beyond pi/2 (clamped), yaw = 0 / pitch = 0 (zero direction components on the centre column and row), distinct times
VIEWS5 = [(0.0, 0.0, 0.0), (0.3, 0.7, 250.0), (2.0, -1.1, 500.0), (-0.45, 3.9, 750.0), (-1.9, 0.2, 1000.0)]


def make_job(N, W, H, y0, y1, preset, accel, algorithm="sphere-tracer"):
    j = N.rm_job()
    j.width, j.height, j.y_start, j.y_end = W, H, y0, y1
    j.camera_pitch, j.camera_yaw, j.time = 0.77, -2.5, 31337.0  # ignored by render_frames
    j.algorithm = N.lib().rm_algorithm_from_string(algorithm.encode())
    j.scene_preset_index = preset
    j.acceleration_structure = ACCEL[accel]
    j.overshoot_factor = j.step_size = float("nan")
    return j


def oracle_frames(oracle, preset, accel, W, H, y0, y1, views, algorithm="sphere-tracer"):
    """Per view: (depth, normal, sdf, iters) of the oracle."""
    sc = oracle.OracleScene(preset=preset, accel=accel)
    out = []
    for pitch, yaw, time in views:
        sc.set_angles(pitch, yaw)
        out.append(sc.render(W, H, y0, y1, algorithm=algorithm, time=time))
    sc.close()
    return out


def oracle_diag(oracle, frame):
    if frame[2].size == 0:
        return dict(NEUTRAL)
    return oracle.diagnostics(frame[2], frame[3])


class Buffers:
    """The five device buffers of n frames of npx pixels plus `guard` pixels behind them, and the accumulators, all
    pre-filled with a sentinel."""

    def __init__(self, n, npx, guard=64, rgba=True):
        import torch
        dev = torch.device("cuda:0")
        self.n, self.npx, self.total = n, npx, n * npx
        size = self.total + guard
        self.depth = torch.full((size,), SENTINEL, dtype=torch.uint8, device=dev)
        self.normal = torch.full((3 * size,), SENTINEL, dtype=torch.uint8, device=dev)
        self.sdf = torch.full((2 * size,), SENTINEL, dtype=torch.uint8, device=dev).view(torch.int16)
        self.iters = torch.full((2 * size,), SENTINEL, dtype=torch.uint8, device=dev).view(torch.int16)
        self.rgba = torch.full((4 * size,), SENTINEL, dtype=torch.uint8, device=dev) if rgba else None
        self.acc = torch.full((32 * (n + 1),), SENTINEL, dtype=torch.uint8, device=dev)

    def pixel_args(self):
        return self.depth, self.normal, self.sdf, self.iters

    def host(self):
        import torch
        torch.cuda.synchronize()
        out = {"depth": self.depth.cpu().numpy(), "normal": self.normal.cpu().numpy(),
               "sdf": self.sdf.cpu().numpy().view(np.uint16), "iters": self.iters.cpu().numpy().view(np.uint16)}
        if self.rgba is not None:
            out["rgba"] = self.rgba.cpu().numpy()
        return out

    def untouched(self):
        h = self.host()
        word = SENTINEL * 0x0101
        return all((h[k] == (word if k in ("sdf", "iters") else SENTINEL)).all() for k in h)

    def acc_guard_untouched(self):
        return bool((self.acc[32 * self.n:].cpu().numpy() == SENTINEL).all())


def check_frames(oracle, ctx, bufs, want, shader_name, what):
    """All of [0, n * npx) is the oracle's, the guard behind it is untouched, accumulator k is the oracle's of frame k."""
    h = bufs.host()
    bpp = {"depth": 1, "normal": 3, "sdf": 1, "iters": 1, "rgba": 4}
    word = SENTINEL * 0x0101
    for k, name in enumerate(NAMES):
        w = np.concatenate([f[k] for f in want])
        g = h[name][:bpp[name] * bufs.total]
        bad = int((g != w).sum())
        assert bad == 0, "%s: %s differs in %d of %d entries" % (what, name, bad, w.size)
        tail = h[name][bpp[name] * bufs.total:]
        assert (tail == (word if name in ("sdf", "iters") else SENTINEL)).all(), "%s: %s written past the last frame" % (what, name)
    if bufs.rgba is not None:
        w = np.concatenate([oracle.shade(shader_name, *f, f[0].size, 1) for f in want])  # (a shade is per pixel: one row)
        diff = np.abs(h["rgba"][:4 * bufs.total].astype(np.int16) - w.astype(np.int16))
        assert diff.max(initial=0) <= (1 if shader_name == "phong" else 0), "%s: rgba off by %d" % (what, diff.max(initial=0))
        assert (h["rgba"][4 * bufs.total:] == SENTINEL).all(), what + ": rgba written past the last frame"
    got = ctx.decode_accs(bufs.acc[:32 * bufs.n])
    for k, f in enumerate(want):
        assert got[k] == oracle_diag(oracle, f), "%s: accumulator %d: %s" % (what, k, got[k])
    assert bufs.acc_guard_untouched(), what + ": accumulator written past the last frame"


@pytest.fixture(scope="module")
def fctx(rm):
    ctx = rm.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", ["sphere-tracer", "adaptive-step-v3"])
@pytest.mark.parametrize("accel", ["None", "Octree", "BVH"])
@pytest.mark.parametrize("preset", [3, 9, 12, 13], ids=["spheres", "boxes-tori", "animated-translate", "mandelbulb"])
def test_every_kernel_family(rm, oracle, fctx, preset, accel, algorithm):
    """70 x 45 (no multiple of a tile, a partial last tile both ways), rows [7, 38), five views with distinct pitch, yaw and
    time, over the three acceleration structures, two marchers and GEN 0 - 3 (spheres; boxes and tori; an operator forest
    with AnimatedTranslate, so the time counts per frame; the Mandelbulb)."""
    from cpu_raymarcher_amd import _native as N
    W, H, y0, y1 = 70, 45, 7, 38
    shader_name = "phong" if algorithm == "sphere-tracer" else "iteration-heatmap"
    want = oracle_frames(oracle, preset, accel, W, H, y0, y1, VIEWS5, algorithm)
    bufs = Buffers(len(VIEWS5), W * (y1 - y0))
    job = make_job(N, W, H, y0, y1, preset, accel, algorithm)
    fctx.render_frames(job, VIEWS5, *bufs.pixel_args(), rgba=bufs.rgba, shader=N.lib().rm_shader_from_string(shader_name.encode()),
                       diag=bufs.acc)
    check_frames(oracle, fctx, bufs, want, shader_name, "preset %d %s %s" % (preset, accel, algorithm))
    # the instantiation the issue says this case covers: ACCEL, OTHER (a marcher other than the sphere tracer), GEN 0 - 3
    gen = {3: 0, 9: 1, 12: 2, 13: 3}[preset]
    name = "frames_kernel<%d, %s, %d>" % (ACCEL[accel], "false" if algorithm == "sphere-tracer" else "true", gen)
    assert fctx.last_kernel() == name, (fctx.last_kernel(), name)
    if preset in (12, 13):  # the time really differs per frame: the same camera at two times gives two pictures
        a, b = oracle_frames(oracle, preset, accel, W, H, y0, y1, [(0.3, 0.7, 250.0), (0.3, 0.7, 1000.0)], algorithm)
        assert any((x != y).any() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def want_33x9(oracle):
    return oracle_frames(oracle, 3, "BVH", 33, 9, 0, 9, VIEWS5)


@pytest.mark.gpu
@pytest.mark.parametrize("v1_block", [64, 256])
@pytest.mark.parametrize("tile_w", [8, 64])
def test_frames_do_not_leak_into_each_other(rm, oracle, want_33x9, tile_w, v1_block):
    """Five 33 x 9 frames into sentinel-filled buffers with every wave-tile and workgroup shape: each byte of [0, 5 W h) is
    the oracle's, the guard behind it keeps the sentinel."""
    from cpu_raymarcher_amd import _native as N
    ctx = rm.Context(0)
    ctx.set_option("tile_w", tile_w)
    ctx.set_option("v1_block", v1_block)
    bufs = Buffers(5, 33 * 9, guard=512)
    ctx.render_frames(make_job(N, 33, 9, 0, 9, 3, "BVH"), VIEWS5, *bufs.pixel_args(), rgba=bufs.rgba, shader=0, diag=bufs.acc)
    check_frames(oracle, ctx, bufs, want_33x9, "normal", "tile_w %d v1_block %d" % (tile_w, v1_block))
    assert ctx.last_kernel().startswith("frames_kernel<2, false, 0>")
    ctx.close()


@pytest.mark.gpu
def test_diagnostics_only(rm, oracle):
    """No pixel buffer at all: 37 views of the analytics sweep (37 is no multiple of anything in the slot scheme) give the
    metric series.  The same call again gives the same, and an ordinary render with attached diagnostics behind it is right
    too (the two schemes do not disturb each other).  (The second call takes the NEXT entries of the context's ring: that a
    frame's last wave leaves its block zeroed is shown where entries are reused,
    test_ring_entries_are_reused_only_when_free_and_left_zeroed.)"""
    import torch
    from cpu_raymarcher_amd import _native as N
    W, H = 64, 40
    ctx = rm.Context(0)
    views = rm.sweep_views(0, 0, 0, 0.015, n=37)
    assert views.shape == (37, 3)
    want = [oracle_diag(oracle, f) for f in oracle_frames(oracle, 3, "BVH", W, H, 0, H, views)]
    job = make_job(N, W, H, 0, H, 3, "BVH")
    dev = torch.device("cuda:0")
    for rep in range(2):
        acc = torch.full((4 * 37 + 4,), -1, dtype=torch.int64, device=dev)
        ctx.render_frames(job, views, None, None, None, None, diag=acc)
        torch.cuda.synchronize()
        assert ctx.decode_accs(acc[:4 * 37]) == want, rep
        assert acc[4 * 37:].cpu().tolist() == [-1] * 4
        assert ctx.last_kernel().startswith("frames_kernel<")
    job.camera_pitch, job.camera_yaw, job.time = 0.2, 0.5, 0.0
    one = torch.full((4,), -1, dtype=torch.int64, device=dev)
    ctx.render_tile(job, None, None, None, None, diag=one)
    torch.cuda.synchronize()
    assert ctx.decode_acc(one) == oracle_diag(oracle, oracle_frames(oracle, 3, "BVH", W, H, 0, H, [(0.2, 0.5, 0.0)])[0])
    ctx.close()


def _sample_check(oracle, ctx, W, views, sample, sdf, iters, acc, what):
    """Frames `sample` of a batch of W x W frames (preset 3, BVH) against the oracle: counters and accumulators."""
    want = oracle_frames(oracle, 3, "BVH", W, W, 0, W, [tuple(views[k]) for k in sample])
    s16, i16 = sdf.cpu().numpy().view(np.uint16), iters.cpu().numpy().view(np.uint16)
    got = ctx.decode_accs(acc)
    npx = W * W
    for k, f in zip(sample, want):
        assert np.array_equal(s16[k * npx:(k + 1) * npx], f[2]) and np.array_equal(i16[k * npx:(k + 1) * npx], f[3]), (what, k)
        assert got[k] == oracle_diag(oracle, f), (what, k, got[k])
    return got


@pytest.mark.gpu
def test_ring_entries_are_reused_only_when_free_and_left_zeroed(rm, oracle):
    """The context's ring of per-frame view records and accumulator blocks holds 4 096 frames.  Batches of 8 x 8 frames (one
    wave each) that reuse it: (1) 4 100 views -- the ring is replaced by one of exactly that size -- twice on one context, so the
    second call adds into the very blocks the first one used (a block its frame's last wave had not left zeroed would give
    wrong sums) after waiting for the first; (2) on a fresh context, two calls of 3 000 views on two streams issued back to back:
    the second wraps onto entries the first still owns and must not disturb it; then a third that wraps again.  A sample
    of frames of every call against the oracle; a repeated call must give the first one's series exactly."""
    import torch
    from cpu_raymarcher_amd import _native as N
    W = 8
    dev = torch.device("cuda:0")
    job = make_job(N, W, W, 0, W, 3, "BVH")

    def run(ctx, views, stream=None):
        n = len(views)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            sdf = torch.full((n * W * W,), -1, dtype=torch.int16, device=dev)
            iters = torch.full((n * W * W,), -1, dtype=torch.int16, device=dev)
            acc = torch.full((4 * n,), -1, dtype=torch.int64, device=dev)
            ctx.render_frames(job, views, None, None, sdf, iters, diag=acc)
        return sdf, iters, acc

    big = rm.sweep_views(-0.6, 0.0, 0.0003, 0.015, n=4100)
    sample = [0, 1, 7, 8, 9, 63, 64, 2047, 2048, 4095, 4096, 4099]
    ctx = rm.Context(0)
    first = run(ctx, big)
    second = run(ctx, big)  # (issued while the first may still run)
    torch.cuda.synchronize()
    a = _sample_check(oracle, ctx, W, big, sample, *first, "4100 views, first call")
    b = _sample_check(oracle, ctx, W, big, sample, *second, "4100 views, the same entries again")
    assert a == b
    assert len({x["total_sdf"] for x in a}) > 1  # a series, not one value
    small = run(ctx, big[:37])  # and a small batch on the blocks both left behind
    torch.cuda.synchronize()
    assert _sample_check(oracle, ctx, W, big, [0, 5, 36], *small, "37 views behind them")[:37] == a[:37]
    ctx.close()

    ctx = rm.Context(0)
    va, vb = big[:3000], big[1100:4100]
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    ra = run(ctx, va, sa)
    rb = run(ctx, vb, sb)  # entries [0, 3000) again: the first call owns them until it is over
    rc = run(ctx, va, sa)
    torch.cuda.synchronize()
    pick = [0, 1, 1095, 1096, 1500, 2999]
    ga = _sample_check(oracle, ctx, W, va, pick, *ra, "stream A")
    gb = _sample_check(oracle, ctx, W, vb, pick, *rb, "stream B")
    gc = _sample_check(oracle, ctx, W, va, pick, *rc, "stream A again")
    assert ga == gc and ga[1100:3000] == gb[:1900]  # (views 1100 .. 2999 are in both sweeps)
    ctx.close()


@pytest.mark.gpu
def test_edges(rm, oracle, fctx):
    """No view, no row, no column: RM_OK, neutral accumulators, pixel buffers untouched.  One view is the oracle's frame."""
    from cpu_raymarcher_amd import _native as N
    W, H = 40, 24
    bufs = Buffers(3, W * H)
    fctx.render_frames(make_job(N, W, H, 0, H, 3, "BVH"), np.zeros((0, 3)), *bufs.pixel_args(), rgba=bufs.rgba, diag=bufs.acc)
    assert bufs.untouched() and (bufs.acc.cpu().numpy() == SENTINEL).all()
    for job in (make_job(N, W, H, 11, 11, 3, "BVH"), make_job(N, W, H, 12, 5, 3, "BVH"), make_job(N, 0, H, 0, H, 3, "BVH")):
        bufs = Buffers(3, 0)
        fctx.render_frames(job, VIEWS5[:3], *bufs.pixel_args(), rgba=bufs.rgba, diag=bufs.acc)
        assert bufs.untouched()
        assert fctx.decode_accs(bufs.acc[:96]) == [NEUTRAL] * 3
        assert bufs.acc_guard_untouched()
    view = [(0.25, -0.6, 0.0)]
    bufs = Buffers(1, W * H)
    fctx.render_frames(make_job(N, W, H, 0, H, 3, "Octree"), view, *bufs.pixel_args(), rgba=bufs.rgba, shader=2, diag=bufs.acc)
    check_frames(oracle, fctx, bufs, oracle_frames(oracle, 3, "Octree", W, H, 0, H, view), "sdf-heatmap", "one view")


@pytest.mark.gpu
@pytest.mark.parametrize("preset,accel", [(3, "BVH"), (9, "Octree")], ids=["spheres", "boxes"])
def test_length_sqrt_mode(rm, oracle, preset, accel):
    """vec3.length = Math.sqrt(x*x + y*y + z*z) on both sides (the oracle's switch is global: restored afterwards)."""
    from cpu_raymarcher_amd import _native as N
    W, H = 48, 30
    ctx = rm.Context(0)
    oracle.lib().ro_set_length_mode(1)
    try:
        ctx.set_option("length", 1)
        want = oracle_frames(oracle, preset, accel, W, H, 0, H, VIEWS5[:3])
        bufs = Buffers(3, W * H)
        ctx.render_frames(make_job(N, W, H, 0, H, preset, accel), VIEWS5[:3], *bufs.pixel_args(), rgba=bufs.rgba, shader=1, diag=bufs.acc)
        check_frames(oracle, ctx, bufs, want, "phong", "length=sqrt preset %d" % preset)
        assert ctx.last_kernel().startswith("frames_kernel<") and "[length=sqrt]" in ctx.last_kernel()
    finally:
        oracle.lib().ro_set_length_mode(0)
        ctx.close()


@pytest.mark.gpu
def test_not_a_render_entry(rm, oracle):
    """An accumulator attached with rm_render_attach_diagnostics survives a render_frames call and is written by the render
    call after it; rm_scene_set_time's value survives too."""
    import torch
    from cpu_raymarcher_amd import _native as N
    W, H = 40, 24
    dev = torch.device("cuda:0")
    ctx = rm.Context(0)
    sc = rm.Scene("BVH", ctx=ctx)
    sc.loadPreset(12)
    ctx.scene_set_time(640.0)
    pt = np.array([[0.4, 0.1, 0.2]], np.float32)
    before = ctx.scene_distance(pt)
    job = make_job(N, W, H, 0, H, 12, "BVH")
    attached = torch.full((4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    ctx._attach_diag(attached)
    bufs = Buffers(2, W * H)
    ctx.render_frames(job, VIEWS5[:2], *bufs.pixel_args(), rgba=bufs.rgba, diag=bufs.acc)
    torch.cuda.synchronize()
    assert attached.cpu().tolist() == [0x5A5A5A5A5A5A5A5A] * 4  # not written by the batch
    after = ctx.scene_distance(pt)
    assert before[0][0] == after[0][0] and before[1][0] == after[1][0]
    osc = oracle.OracleScene(preset=12, accel="BVH")
    assert after[0][0] == osc.distance(pt[0], time=640.0)[0] != osc.distance(pt[0], time=0.0)[0]
    osc.close()
    job.camera_pitch, job.camera_yaw, job.time = 0.1, 0.4, 100.0
    one = torch.zeros(4 * W * H, dtype=torch.uint8, device=dev)
    ctx.render_tile(job, None, None, None, None, rgba=one)  # still attached: this call takes it
    torch.cuda.synchronize()
    assert ctx.decode_acc(attached) == oracle_diag(oracle, oracle_frames(oracle, 12, "BVH", W, H, 0, H, [(0.1, 0.4, 100.0)])[0])
    check_frames(oracle, ctx, bufs, oracle_frames(oracle, 12, "BVH", W, H, 0, H, VIEWS5[:2]), "normal", "batch before the render")
    ctx.close()


# ---------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("start,delta", [((0.0, 0.0), (0.0, 0.015)), ((1.2, -0.3), (0.05, 0.015)), ((-1.0, 7.0), (-0.07, -0.3)),
                                         ((3.0, 1.0), (-0.2, 0.1))])
def test_sweep_views_is_the_mirror_camera(rm, start, delta):
    """views[k] = Camera.setAngles followed by k x Camera.rotateCamera, bit for bit: sequential additions, the pitch clamp at
    every step (the second and third sweeps run into it, the fourth starts beyond it)."""
    n = 51
    got = rm.sweep_views(start[0], start[1], delta[0], delta[1], time0=2.5, d_time=0.1, n=n)
    cam = rm.Camera()
    cam.setAngles(*start)
    clamped = 0
    for k in range(n):
        if k:
            cam.rotateCamera(*delta)
        pitch, yaw = cam.getAngles()
        assert got[k, 0] == pitch and got[k, 1] == yaw and got[k, 2] == 2.5 + k * 0.1, k
        clamped += abs(pitch) == math.pi / 2
    if delta[0]:
        assert clamped > 3
    if delta == (0.0, 0.015):
        assert got[50, 1] != 50 * 0.015  # the sequential sum, not the product (they differ in the last bits here)


def test_sweep_views_refuses_bad_arguments(rm):
    from cpu_raymarcher_amd import _native as N
    L = N.lib()
    out = np.zeros((4, 3))
    p = out.ctypes.data_as(C.c_void_p)
    assert L.rm_sweep_views(0.0, 0.0, 0.0, 0.1, 0.0, 0.0, 4, p) == N.RM_OK
    assert L.rm_sweep_views(0.0, 0.0, 0.0, 0.1, 0.0, 0.0, 0, None) == N.RM_OK
    for bad in range(6):
        for v in (float("nan"), float("inf")):
            args = [0.0, 0.0, 0.0, 0.1, 0.0, 0.0]
            args[bad] = v
            assert L.rm_sweep_views(*args, 4, p) == N.RM_E_INVALID, (bad, v)
    assert L.rm_sweep_views(0.0, 0.0, 0.0, 0.1, 0.0, 0.0, -1, p) == N.RM_E_INVALID
    assert L.rm_sweep_views(0.0, 0.0, 0.0, 0.1, 0.0, 0.0, 4, None) == N.RM_E_INVALID
    with pytest.raises(N.RmError):
        rm.sweep_views(0, 0, 0, float("nan"), n=3)
    assert rm.sweep_views(0, 0, 0, 0.1, n=0).shape == (0, 3)


@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_frames_kernels_spill_no_vgpr(extra):
    """The 24 frames_kernel<ACCEL, OTHER, GEN> instantiations of either vec3.length build, on the compiler's own listing (the
    compile test_build_invariants.py makes, shared with it): no VGPR spill; no scratch for spheres and primitive lists; the
    interpreter's bound for the expression programs, as for render_kernel."""
    import test_build_invariants as B
    if not B.os.path.exists(B.HIPCC) or B.shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = B.resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void frames_kernel<")}
    assert len(kernels) == 24, sorted(usage)
    B.assert_no_vgpr_spill(kernels, 800)


def test_host_only_context(rm):
    """RM_E_NO_DEVICE without a device; the argument checks come first and need none."""
    from cpu_raymarcher_amd import _native as N
    L = N.lib()
    ctx = rm.Context(None)
    job = make_job(N, 64, 40, 0, 40, 3, "BVH")
    views = rm.sweep_views(0, 0, 0, 0.015, n=4)
    p = views.ctypes.data_as(C.c_void_p)
    nul = [None] * 7  # five pixel buffers, the accumulators, the stream

    def call(job_ref, vp, n):
        return L.rm_render_frames_device(ctx._h, job_ref, 0, vp, n, *nul)

    assert call(C.byref(job), p, 4) == N.RM_E_NO_DEVICE
    assert call(C.byref(job), None, 0) == N.RM_E_NO_DEVICE
    assert call(None, p, 4) == N.RM_E_INVALID
    assert call(C.byref(job), p, -1) == N.RM_E_INVALID
    assert call(C.byref(job), p, 65536) == N.RM_E_INVALID
    assert call(C.byref(job), None, 4) == N.RM_E_INVALID
    for col in range(3):
        for v in (float("nan"), float("-inf")):
            bad = views.copy()
            bad[2, col] = v
            assert call(C.byref(job), bad.ctypes.data_as(C.c_void_p), 4) == N.RM_E_INVALID, (col, v)
    assert L.rm_render_frames_device(None, C.byref(job), 0, p, 4, *nul) == N.RM_E_INVALID
    with pytest.raises(N.RmError) as e:
        ctx.render_frames(job, views, None, None, None, None)
    assert e.value.code == N.RM_E_NO_DEVICE
    ctx.close()
