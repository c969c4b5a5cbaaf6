"""The bundle cull by leaf screen rectangles (rm_render_v2.hip, option `rect_cull`) on the device.

The cull only selects candidates for the exact slab test, and a batch without a candidate takes the result the exact test would
have given every ray of it: any difference is a bug.  Every check is byte equality of depth, normal, SDF evaluations, iterations,
shaded RGBA and the four fused diagnostics between the wave loop with `rect_cull` 1, with `rect_cull` 0 (the plane cull) and the
one-ray-per-lane kernel (the tree walk).  Every case also reads back which cull the launch used (rm_debug_rect_cull): a launch
that silently took the plane cull does not pass as a test of the rectangles.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("depth", "normal", "sdf", "iters", "rgba", "diagnostics")
DEFAULTS = dict(kernel=2, rect_cull=1, cull=1, specialise=1, specialise_v2_after=0, item_px=128, blocks_per_cu=6, refill=64, lpt=1)
V2_AOT = "render_kernel_v2<"
V2_RTC = "[launch constants compiled in]"
GOLDEN = (0.0, 0.0)
CAMERAS = [GOLDEN, (0.2, 0.3), (0.0, 1.2)]  # (pitch, yaw)


def _scene(name):
    """(centres float32 [n, 3], radii float64 [n]) of a named upload, or the preset's index."""
    if name == "dense":
        return 3
    if name == "grid9":
        return 2
    rng = np.random.default_rng(5)
    if name == "random300":  # 172 leaves: three 64-leaf trips of the cull loop
        return rng.uniform(-1.5, 1.5, (300, 3)).astype(np.float32), rng.uniform(0.03, 0.1, 300)
    if name == "random2000":  # more leaves than the cull's table holds: no bundle cull at all
        return rng.uniform(-1.5, 1.5, (2000, 3)).astype(np.float32), rng.uniform(0.01, 0.04, 2000)
    if name == "around_camera":
        # the camera of angles (0, 0) sits at (0, 0, 3): inside this scene's root box, and inside the leaf box (centre -+ 1.5 r)
        # of the sphere beside it, whose surface it is outside of; at other angles it orbits through the cloud
        c = rng.uniform(-1.2, 1.2, (90, 3)).astype(np.float32)
        c[:, 2] = rng.uniform(0.5, 3.6, 90).astype(np.float32)
        keep = np.linalg.norm(c - np.array([0, 0, 3], np.float32), axis=1) > 0.45
        c = np.concatenate([c[keep], np.array([[0.3, 0.0, 3.0]], np.float32)])
        r = np.concatenate([rng.uniform(0.05, 0.12, int(keep.sum())), [0.25]])
        return c, r
    raise KeyError(name)


class Renders:
    """One context for the module; a reference frame is rendered once per (scene, camera, size, kind) and shared."""

    def __init__(self, rm):
        import torch
        self.rm, self.torch = rm, torch
        self.ctx = rm.Context(0)
        self.dev = torch.device("cuda:0")
        self.refs = {}

    def scene(self, name, ang, **opts):
        for k, v in dict(DEFAULTS, **opts).items():
            self.ctx.set_option(k, v)
        sc = self.rm.Scene("BVH", ctx=self.ctx)
        sp = _scene(name)
        if isinstance(sp, int):
            sc.loadPreset(sp)
        else:
            sc.loadSpheres(*sp)
        sc.camera.setAngles(*ang)
        return sc

    def buffers(self, n):
        t = self.torch
        return [t.zeros(n, dtype=t.uint8, device=self.dev), t.zeros(3 * n, dtype=t.uint8, device=self.dev),
                t.zeros(n, dtype=t.int16, device=self.dev), t.zeros(n, dtype=t.int16, device=self.dev),
                t.zeros(4 * n, dtype=t.uint8, device=self.dev), t.full((4,), -1, dtype=t.int64, device=self.dev)]

    def host(self, b):
        return (b[0].cpu().numpy(), b[1].cpu().numpy(), b[2].cpu().numpy().view(np.uint16), b[3].cpu().numpy().view(np.uint16),
                b[4].cpu().numpy(), self.ctx.decode_acc(b[5]))

    def planned(self, ang, size):
        rot, origin = self.rm.context.camera_from_angles(*ang)
        return self.ctx.rect_cull(rot, origin, *size)["planned"]

    def gpu(self, name, ang, size, launches=1, **opts):
        """(depth, normal, sdf, iters, rgba, diagnostics) of one frame, the kernel that rendered it, whether it culled by rectangles."""
        sc = self.scene(name, ang, **opts)
        W, H = size
        b = self.buffers(W * H)
        planned = self.planned(ang, size)
        for _ in range(launches):  # (the run-time compiled kernel takes over after some launches)
            self.rm.SphereTracer().runRaymarcher(sc, b[0], b[1], b[2], b[3], W, H, 0.0, shadedBuffer=b[4], shader="iteration-heatmap",
                                                 diagnostics=b[5])
            self.torch.cuda.synchronize()
        rot, origin = self.rm.context.camera_from_angles(*ang)
        used = self.ctx.rect_cull(rot, origin, W, H)["last"]
        if self.ctx.get_option("kernel") == 2:
            assert used == planned  # the read that needs no device says what the launcher then did
        return self.host(b), self.ctx.last_kernel(), used

    def reference(self, name, ang, size, which):
        """`which`: "planes" (the wave loop with rect_cull 0) or "walk" (the one-ray-per-lane kernel), ahead-of-time kernels."""
        key = (name, ang, size, which)
        if key not in self.refs:
            opts = dict(rect_cull=0) if which == "planes" else dict(kernel=1)
            frame, kernel, used = self.gpu(name, ang, size, specialise=0, **opts)
            assert ((V2_AOT in kernel) == (which == "planes")) and V2_RTC not in kernel and (which == "walk" or not used), (kernel, used)
            for a in frame[:5]:
                a.setflags(write=False)
            self.refs[key] = frame
        return self.refs[key]


@pytest.fixture(scope="module")
def renders(rm):
    r = Renders(rm)
    yield r
    r.ctx.close()


def same(got, want, what, names=NAMES):
    for name, g, w in zip(NAMES, got, want):
        if name not in names:
            continue
        if name == "diagnostics":
            assert g == w, "%s: diagnostics %s, expected %s" % (what, g, w)
        else:
            bad = int((g != w).sum())
            assert bad == 0, "%s: %s differs in %d of %d entries" % (what, name, bad, w.size)


def check(renders, name, ang, size, rects=True, v2=V2_AOT, **opts):
    got, kernel, used = renders.gpu(name, ang, size, **opts)
    assert v2 in kernel and (v2 == V2_RTC or V2_RTC not in kernel), kernel
    assert used == rects, "%s: the launch %s the leaf rectangles" % (name, "used" if used else "did not use")
    for which in ("planes", "walk"):
        same(got, renders.reference(name, ang, size, which), "%s camera %s %s %s: against %s" % (name, ang, size, opts, which))
    return got


@pytest.mark.parametrize("ang", CAMERAS, ids=lambda a: "pitch%g-yaw%g" % a)
def test_dense_sphere_grid(renders, ang):
    check(renders, "dense", ang, (256, 144))


@pytest.mark.parametrize("opts", [dict(item_px=64), dict(item_px=256), dict(blocks_per_cu=1), dict(refill=24), dict(item_px=64, tile_w=16)],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
def test_dense_sphere_grid_partial_tiles_and_launch_options(renders, opts):
    """250 x 130: edges that are no multiple of the tile.  `refill` 24: batches that are not whole, beside the ones that are."""
    try:
        check(renders, "dense", (0.2, 0.3), (250, 130), **opts)
    finally:
        renders.ctx.set_option("tile_w", 8)


def test_grid_of_nine_spheres(renders):
    for ang in (GOLDEN, (0.2, 0.3)):
        check(renders, "grid9", ang, (250, 130))


def test_several_trips_of_the_cull_loop(renders):
    renders.scene("random300", GOLDEN)
    assert 128 < renders.ctx.scene_info()["bvh_leaves"] <= 256
    for ang in (GOLDEN, (0.0, 1.2)):
        check(renders, "random300", ang, (250, 130))


def test_camera_inside_the_root_box_and_inside_a_leaf(renders):
    """Leaves with corners behind the camera keep the whole frame."""
    sc = renders.scene("around_camera", GOLDEN)
    rot, origin = renders.rm.context.camera_from_angles(*GOLDEN)
    info = renders.ctx.scene_info()
    assert all(info["root_min"][k] < origin[k] < info["root_max"][k] for k in range(3))
    rects, _ = renders.ctx.leaf_rects(rot, origin, 250, 130)
    assert (rects == np.array([0, 65535, 0, 65535], np.uint16)).all(axis=1).any()
    for ang in (GOLDEN, (0.2, 0.3), (0.0, 1.2)):
        check(renders, "around_camera", ang, (250, 130))
    del sc


def test_scene_beyond_the_leaf_cap_has_no_rectangles(renders):
    check(renders, "random2000", (0.2, 0.3), (250, 130), rects=False)


def test_two_cameras_in_flight_on_two_streams(renders):
    """The table belongs to the launch: two renders of one scene, the camera turned in between, on different streams."""
    torch, rm = renders.torch, renders.rm
    W, H = 256, 144
    sc = renders.scene("dense", (0.2, 0.3))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs, angles = [renders.buffers(W * H) for _ in range(6)], []
    torch.cuda.synchronize()  # (the buffers are cleared on the default stream, which the two streams do not wait for)
    for rep in range(3):  # (several pairs: the launches do overlap)
        for s in streams:
            b = bufs[len(angles)]
            with torch.cuda.stream(s):
                rm.SphereTracer().runRaymarcher(sc, b[0], b[1], b[2], b[3], W, H, 0.0, shadedBuffer=b[4], shader="iteration-heatmap",
                                                diagnostics=b[5])
            angles.append((sc.camera.pitch, sc.camera.yaw))
            sc.camera.rotateCamera(-0.2, 0.9)
    torch.cuda.synchronize()
    assert renders.ctx.rect_cull(*rm.context.camera_from_angles(0.2, 0.3), W, H)["last"]
    for b, ang in zip(bufs, angles):
        same(renders.host(b), renders.reference("dense", ang, (W, H), "planes"), "in flight, camera %s" % (ang,))


def test_striped_launches(renders):
    """stripe_rows 16, three parts, and a stripe list: the rows a batch covers are not consecutive rows of the frame."""
    from cpu_raymarcher_amd.host import _job
    rm, ctx = renders.rm, renders.ctx
    W, H, SR = 250, 130, 16
    ang = (0.2, 0.3)
    ref = renders.reference("dense", ang, (W, H), "planes")
    sc = renders.scene("dense", ang)
    job = _job(sc, W, H, 0.0, 0, H, "sphere-tracer")
    n_stripes = (H + SR - 1) // SR
    lists = [list(range(p, n_stripes, 3)) for p in range(3)] + [[0, 1, 4, 8]]
    for k, ids in enumerate(lists):
        rows = np.concatenate([np.arange(i * SR, min(H, (i + 1) * SR)) for i in ids])
        b = renders.buffers(len(rows) * W)
        if k < 3:
            ctx.render_stripes(job, SR, 3, k, b[0], b[1], b[2], b[3], rgba=b[4], shader=rm._native.lib().rm_shader_from_string(b"iteration-heatmap"), diag=b[5])
        else:
            ctx.render_stripe_list(job, SR, ids, b[0], b[1], b[2], b[3], rgba=b[4], shader=rm._native.lib().rm_shader_from_string(b"iteration-heatmap"), diag=b[5])
        renders.torch.cuda.synchronize()
        assert ctx.rect_cull(*rm.context.camera_from_angles(*ang), W, H)["last"]
        got = renders.host(b)
        for name, g, w, per in zip(NAMES[:5], got, ref, (1, 3, 1, 1, 4)):
            assert np.array_equal(g.reshape(len(rows), W * per), w.reshape(H, W * per)[rows]), "stripes %s: %s" % (ids, name)
        sdf = got[2].astype(np.int64)
        assert got[5] == {"total_sdf": int(sdf.sum()), "total_iters": int(got[3].astype(np.int64).sum()), "max_sdf": int(sdf.max()),
                          "min_sdf": int(sdf.min())}


def test_golden_crop_of_the_rotated_dense_grid(renders, golden, golden_crops):
    name = "C3r_dense_540p_bvh_rotated_sdfheat"
    cfg, c = golden[name]["config"], golden[name]["crop"]
    W, H = cfg["width"], cfg["height"]
    got, kernel, used = renders.gpu("dense", (cfg["pitch"], cfg["yaw"]), (W, H))
    assert V2_AOT in kernel and used
    idx = (np.arange(c["y"], c["y"] + c["size"])[:, None] * W + np.arange(c["x"], c["x"] + c["size"])[None, :]).ravel()
    for k, key in ((2, "sdf"), (3, "iters"), (0, "depth")):
        assert np.array_equal(got[k][idx], golden_crops[name + "/" + key]), key
    for k, v in golden[name]["diagnostics"].items():
        assert got[5][k] == v, (k, got[5][k], v)


@pytest.mark.parametrize("rect_cull", [1, 0])
def test_run_time_compiled_wave_loop(renders, rect_cull):
    """The copy of the wave loop compiled with the launch constants as literals, `rect_cull` among them, on either side of the
    switch: it must be the kernel that ran (accepted, not refused for spills)."""
    got, kernel, used = renders.gpu("dense", (0.2, 0.3), (250, 130), launches=3, specialise_v2_after=1, rect_cull=rect_cull)
    assert V2_RTC in kernel, kernel
    assert used == bool(rect_cull)
    for which in ("planes", "walk"):
        same(got, renders.reference("dense", (0.2, 0.3), (250, 130), which), "compiled, rect_cull %d: against %s" % (rect_cull, which))
