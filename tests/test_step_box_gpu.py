"""In-round march steps against the step-box table (rm_render_v2.hip, section M, option `step_box`).

A step taken inside a round is the ordinary path's step or it is a bug, so every check is byte equality of depth, normal, SDF
evaluations, iterations, shaded RGBA and the four fused diagnostics between the wave loop with `step_box` 1, with `step_box` 0
(the exact leaf-set test), with `multi_step` 0 (no in-round step) and the CPU oracle.  Every case also reads back which test the
launch used (rm_debug_step_box): a launch that silently took the exact test does not pass as a test of the table.

Frames are 200 x 136 (the rays of column 100 have d.x == 0; partial tiles both ways, several workgroups)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = (200, 136)
NAMES = ("depth", "normal", "sdf", "iters", "rgba", "diagnostics")
DEFAULTS = dict(kernel=2, multi_step=1, step_box=1, specialise=1, specialise_v2_after=0, list_cap=32, lds_kb=0, length=0, uniform=1, rel=1)
V2_AOT = "render_kernel_v2<"
V2_RTC = "[launch constants compiled in]"
GOLDEN = (0.0, 0.0)


def _nine():
    g = np.array([[x, y, 0.0] for y in (-0.9, 0.0, 0.9) for x in (-0.9, 0.0, 0.9)])
    return np.concatenate([g, np.linspace(0.22, 0.47, 9).reshape(-1, 1)], axis=1).astype(np.float32)


def _scene(name):
    """float32 [n, 4] spheres of a named scene, or the preset's index."""
    if name == "dense":
        return 3
    if name == "grid9":
        return 2
    if name == "face_plane":
        # the camera of angles (0, 0) sits on the z axis: the rays of column W / 2 run in the plane x = 0.  A sphere's box is its
        # centre -+ 1.5 r: with r a binary fraction and |centre x| = 1.5 r the boxes on the right have a face lo.x == 0 and those
        # on the left a face hi.x == 0, exactly, and those rays run IN that face from leaf to leaf.  The sphere of radius 0.5
        # centred at x = 0.5 touches the plane at the origin: the same rays graze it and take long runs of in-round steps.
        return np.array([[0.5, 0.0, 0.0, 0.5], [0.75, 1.3, -0.3, 0.5], [0.375, 1.9, 0.4, 0.25], [0.5625, -1.4, 0.3, 0.375],
                         [0.1875, -2.0, -0.2, 0.125], [-0.75, 1.2, 0.5, 0.5], [-0.375, 2.0, -0.4, 0.25], [-0.5625, -1.3, -0.5, 0.375],
                         [-0.1875, -1.9, 0.6, 0.125], [0.0, 0.0, -1.5, 0.4]], np.float32)
    if name == "skim":  # tall and thin: most rays run along the long faces of the root box and leave it in mid-run
        y = np.linspace(-2.4, 2.4, 25)
        g = np.stack([0.05 * np.sin(7.0 * y), y, 0.05 * np.cos(5.0 * y)], axis=1)
        return np.concatenate([g, np.full((25, 1), 0.11) + 0.02 * np.cos(3.0 * y).reshape(-1, 1)], axis=1).astype(np.float32)
    if name == "over_capacity":  # 5 x 5 x 5 with random radii: more than 62 distinct thresholds per axis, no table
        a = np.linspace(-1.2, 1.2, 5)
        g = np.array([[x, y, z] for z in a for y in a for x in a])
        return np.concatenate([g, np.random.default_rng(8).uniform(0.08, 0.3, (125, 1))], axis=1).astype(np.float32)
    if name == "close_faces":  # two spheres whose faces differ by 1e-4 on x: several thresholds in one look-up bin
        return np.concatenate([_nine(), np.array([[0.0, 1.9, 0.3, 0.3], [1e-4, -1.9, 0.3, 0.3]], np.float32)])
    raise KeyError(name)


class Renders:
    """One context for the module; a reference frame is rendered once per (scene, camera, length) and shared."""

    def __init__(self, rm, oracle):
        import torch
        self.rm, self.oracle, self.torch = rm, oracle, torch
        self.ctx = rm.Context(0)
        self.dev = torch.device("cuda:0")
        self.refs = {}

    def gpu(self, name, ang, launches=1, **opts):
        """(depth, normal, sdf, iters, rgba, diagnostics) of one frame, the kernel that rendered it, and whether it used the table."""
        torch, ctx = self.torch, self.ctx
        for k, v in dict(DEFAULTS, **opts).items():
            ctx.set_option(k, v)
        sc = self.rm.Scene("BVH", ctx=ctx)
        sp = _scene(name)
        if isinstance(sp, int):
            sc.loadPreset(sp)
        else:
            sc.loadSpheres(sp[:, :3], sp[:, 3])
        sc.camera.setAngles(*ang)
        W, H = SIZE
        n = W * H
        d = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        nr = torch.zeros(3 * n, dtype=torch.uint8, device=self.dev)
        s16 = torch.zeros(n, dtype=torch.int16, device=self.dev)
        i16 = torch.zeros(n, dtype=torch.int16, device=self.dev)
        rgba = torch.zeros(4 * n, dtype=torch.uint8, device=self.dev)
        acc = torch.full((4,), -1, dtype=torch.int64, device=self.dev)
        tracer = self.rm.SphereTracer()
        planned = ctx.step_box()["planned"]
        for _ in range(launches):  # (the run-time compiled kernel takes over after some launches)
            tracer.runRaymarcher(sc, d, nr, s16, i16, W, H, 0.0, shadedBuffer=rgba, shader="iteration-heatmap", diagnostics=acc)
            torch.cuda.synchronize()
        used = ctx.step_box()["last"]
        assert used == planned  # the read that needs no device says what the launcher then did
        out = (d.cpu().numpy(), nr.cpu().numpy(), s16.cpu().numpy().view(np.uint16), i16.cpu().numpy().view(np.uint16),
               rgba.cpu().numpy(), ctx.decode_acc(acc))
        return out, ctx.last_kernel(), used

    def reference(self, name, ang, length, which):
        """`which`: "exact" (step_box 0), "single" (multi_step 0), both from the ahead-of-time kernel, or "oracle"."""
        key = (name, ang, length, which)
        if key not in self.refs:
            if which == "oracle":
                O = self.oracle
                sp = _scene(name)
                O.lib().ro_set_length_mode(length)
                try:
                    sc = O.OracleScene(preset=sp if isinstance(sp, int) else None, accel="BVH", spheres=None if isinstance(sp, int) else sp)
                    sc.set_angles(*ang)
                    bufs = sc.render(*SIZE)
                    rgba = O.shade("iteration-heatmap", *bufs, *SIZE)
                finally:
                    O.lib().ro_set_length_mode(0)
                sdf, it = bufs[2].astype(np.int64), bufs[3].astype(np.int64)
                diag = {"total_sdf": int(sdf.sum()), "total_iters": int(it.sum()), "max_sdf": int(sdf.max()), "min_sdf": int(sdf.min())}
                frame = bufs + (rgba, diag)
            else:
                opts = dict(step_box=0) if which == "exact" else dict(multi_step=0)
                frame, kernel, used = self.gpu(name, ang, length=length, specialise=0, **opts)
                assert V2_AOT in kernel and V2_RTC not in kernel and not used, (kernel, used)
            for a in frame[:5]:
                a.setflags(write=False)
            self.refs[key] = frame
        return self.refs[key]


@pytest.fixture(scope="module")
def renders(rm, oracle):
    r = Renders(rm, oracle)
    yield r
    r.ctx.close()


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if name == "diagnostics":
            assert g == w, "%s: diagnostics %s, expected %s" % (what, g, w)
        else:
            bad = int((g != w).sum())
            assert bad == 0, "%s: %s differs in %d of %d entries" % (what, name, bad, w.size)


def check(renders, name, ang, table=True, v2=V2_AOT, length=0, **opts):
    """A frame with `step_box` 1 against the three references; `table`: whether the launch must have used the table."""
    got, kernel, used = renders.gpu(name, ang, length=length, **opts)
    assert v2 in kernel and (v2 == V2_RTC or V2_RTC not in kernel), kernel
    if length:
        assert "[length=sqrt]" in kernel, kernel
    assert used == table, "%s: the launch %s the step-box table" % (name, "used" if used else "did not use")
    what = "%s camera %s %s" % (name, ang, opts)
    for which in ("exact", "single", "oracle"):
        same(got, renders.reference(name, ang, length, which), "%s: against %s" % (what, which))
    return got


@pytest.mark.parametrize("ang", [GOLDEN, (0.4, 0.3), (-0.4, 0.785)], ids=lambda a: "pitch%g-yaw%g" % a)
def test_dense_sphere_grid(renders, ang):
    check(renders, "dense", ang)


def test_dense_sphere_grid_length_sqrt(renders):
    check(renders, "dense", (0.4, 0.3), length=1)


def test_grid_of_nine_spheres(renders):
    check(renders, "grid9", GOLDEN)
    check(renders, "grid9", (0.3, 0.7))


def test_rays_in_a_leaf_face_plane(renders):
    """The rays of column W / 2 have d.x == 0 and x == 0: every point of theirs is ON the face x = 0 of leaf boxes -- on the
    threshold lo.x of some, one binary32 below the threshold nextup(hi.x) of others."""
    ctx = renders.ctx
    got = check(renders, "face_plane", GOLDEN)
    nodes = ctx.scene_table("bvh").reshape(-1, 32)
    lo, hi, leaf = nodes[:, 0:12].copy().view("<f4"), nodes[:, 16:28].copy().view("<f4"), nodes[:, 28:32].copy().view("<i4").reshape(-1)
    full = (leaf >= 0) & ((leaf & 0xFF) != 0)
    assert (lo[full, 0] == 0.0).any() and (hi[full, 0] == 0.0).any()  # leaf faces at x = 0 exactly, from either side
    o, d = renders.rm.camera_rays(SIZE[0], SIZE[1], *GOLDEN)
    assert np.all(d.reshape(SIZE[1], SIZE[0], 3)[:, SIZE[0] // 2, 0] == 0.0) and o[0] == 0.0
    iters = got[3].reshape(SIZE[1], SIZE[0])
    assert iters[:, SIZE[0] // 2].max() >= 20  # the grazing rays of that column do march
    check(renders, "face_plane", (0.0, 0.785))


def test_rays_that_leave_the_root_box_in_mid_run(renders):
    for ang in (GOLDEN, (1.2, 0.785)):
        check(renders, "skim", ang)


def test_scene_without_a_table_takes_the_exact_test(renders):
    check(renders, "over_capacity", (0.3, 0.7), table=False)


def test_several_thresholds_in_one_bin(renders):
    check(renders, "close_faces", GOLDEN)
    check(renders, "close_faces", (0.4, 0.3), uniform=0, rel=0)


def test_no_room_for_the_table_in_lds(renders):
    """A budget and a hit-list capacity that the scene's tables just reach: the table would cost the budget, the launch runs
    without it (and one with a little more room runs with it)."""
    ctx = renders.ctx
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.scene_from_preset(3, 2)
    found = None
    for kb in range(16, 65):
        for cap in range(1, 13):
            ctx.set_option("lds_kb", kb)
            ctx.set_option("list_cap", cap)
            if found is None and ctx.step_box()["reason"] == 3:
                found = (kb, cap)
    assert found is not None
    check(renders, "dense", (0.4, 0.3), table=False, lds_kb=found[0], list_cap=found[1])
    check(renders, "dense", (0.4, 0.3), table=True, lds_kb=16, list_cap=16)


@pytest.mark.parametrize("step_box", [1, 0])
def test_run_time_compiled_wave_loop(renders, step_box):
    """The copy of the wave loop compiled with the launch constants as literals -- `step_box`, the table's geometry and its place
    in LDS among them -- on either side of the switch: it must be the kernel that ran (accepted, not refused for spills)."""
    got, kernel, used = renders.gpu("dense", (0.4, 0.3), launches=3, specialise_v2_after=1, step_box=step_box)
    assert V2_RTC in kernel, kernel
    assert used == bool(step_box)
    for which in ("exact", "single", "oracle"):
        same(got, renders.reference("dense", (0.4, 0.3), 0, which), "compiled, step_box %d: against %s" % (step_box, which))
