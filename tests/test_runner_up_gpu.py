"""Section M's runner-up test (rm_render_v2.hip, option `runner_up`): a step the one bound of all other candidates refuses is
taken when the runner-up sphere's own distance at the new point, and the third key's bound less the distance travelled, both
exceed the winner's exact distance.

The rule only changes which round a march step is taken in, so every check is equality of bits: depth, normal, SDF evaluations,
iterations, shaded RGBA and the fused diagnostics with `runner_up` 1 against `runner_up` 0, against `multi_step` 0 and against the
CPU oracle, with vec3.length = hypot and sqrt, from the library's kernel and from the run-time compiled copy.  Every frame reads
back whether its launch applied the rule (rm_debug_runner_up): a launch that went the old way does not pass as a test of it.

Scenes: the Dense Sphere Grid, the Grid of Spheres, the lattice around the camera; two equal spheres (a runner-up, nothing behind
it: lb3 infinite); two equal overlapping spheres placed symmetrically about the view axis (equal distances on the symmetry plane:
the near tie the exact evaluation's redo and the rule's strict compare must both leave alone); four equal spheres close enough
for the grown boxes of their leaves to overlap (a BVH leaf holds at most two spheres, so a finite lb3 needs candidates from two
leaves).  Controls that must report the rule as not taken: one sphere and three unequal spheres (no one-radius launch), and
`cell_tab` 0.  Frames are 160 x 90, and 96 x 54 (partial tiles); cameras (0, 0) and one rotated view.

The small frames exercise the rule: it acts per ray, wherever a ray passes between two spheres of a grid, and at 4K it keeps 0.60
lane steps per pixel of the Dense Grid that the one bound refuses (profiles/NOTES.md, round 12; scripts/in_round_model.c)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("depth", "normal", "sdf", "iters", "rgba", "diagnostics")
DEFAULTS = dict(kernel=2, multi_step=1, step_box=1, cell_tab=1, runner_up=1, specialise=1, specialise_v2_after=0, list_cap=32, lds_kb=0, length=0,
                uniform=1, rel=1)
V2_AOT = "render_kernel_v2<"
V2_RTC = "[launch constants compiled in]"
GOLDEN = (0.0, 0.0)
ROTATED = (0.4, 0.3)
SIZES = ((160, 90), (96, 54))


def _lattice(centre):
    a = np.linspace(-1.2, 1.2, 5)
    g = np.array([[x, y, z] for x in a for y in a for z in a]) + np.asarray(centre)
    return np.concatenate([g, np.full((125, 1), 0.15)], axis=1).astype(F)


def _scene(name):
    """float32 [n, 4] spheres of a named scene, or the preset's index."""
    if name == "dense":
        return 3
    if name == "grid9":
        return 2
    if name == "around_camera":  # the camera of angles (0, 0) sits at (0, 0, 3): between the spheres of this lattice
        return _lattice((0.3, 0.3, 3.3))
    if name == "one":
        return np.array([[0.1, -0.1, 0.0, 0.5]], F)
    if name == "two_equal":
        return np.array([[-0.7, 0.0, 0.0, 0.4], [0.7, 0.1, 0.2, 0.4]], F)
    if name == "two_symmetric":  # the camera looks down -z from (0, 0, 3): the plane x = 0 is equally far from both
        return np.array([[-0.25, 0.0, 0.0, 0.4], [0.25, 0.0, 0.0, 0.4]], F)
    if name == "four_equal":
        return np.array([[-0.3, -0.3, 0.0, 0.35], [0.3, -0.3, 0.1, 0.35], [-0.3, 0.3, 0.1, 0.35], [0.3, 0.3, 0.0, 0.35]], F)
    if name == "three_unequal":
        return np.array([[-0.5, 0.0, 0.0, 0.4], [0.1, 0.2, 0.0, 0.35], [0.6, -0.1, 0.2, 0.45]], F)
    raise KeyError(name)


class Renders:
    """One context for the module; a frame is rendered once per (scene, camera, size, options) and shared."""

    def __init__(self, rm, oracle):
        import torch
        self.rm, self.oracle, self.torch = rm, oracle, torch
        self.ctx = rm.Context(0)
        self.dev = torch.device("cuda:0")
        self.frames = {}

    def gpu(self, name, ang, size, launches=1, **opts):
        """((depth, normal, sdf, iters, rgba, diagnostics), kernel name, whether the launch applied the rule, why not)."""
        key = (name, ang, size, launches, tuple(sorted(opts.items())))
        if key in self.frames:
            return self.frames[key]
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
        W, H = size
        n = W * H
        d = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        nr = torch.zeros(3 * n, dtype=torch.uint8, device=self.dev)
        s16 = torch.zeros(n, dtype=torch.int16, device=self.dev)
        i16 = torch.zeros(n, dtype=torch.int16, device=self.dev)
        rgba = torch.zeros(4 * n, dtype=torch.uint8, device=self.dev)
        acc = torch.full((4,), -1, dtype=torch.int64, device=self.dev)
        tracer = self.rm.SphereTracer()
        plan = ctx.runner_up()
        for _ in range(launches):  # (the run-time compiled kernel takes over after some launches)
            tracer.runRaymarcher(sc, d, nr, s16, i16, W, H, 0.0, shadedBuffer=rgba, shader="iteration-heatmap", diagnostics=acc)
            torch.cuda.synchronize()
        used = ctx.runner_up()["last"]
        assert used == plan["planned"]  # the read that needs no device says what the launcher then did
        out = (d.cpu().numpy(), nr.cpu().numpy(), s16.cpu().numpy().view(np.uint16), i16.cpu().numpy().view(np.uint16),
               rgba.cpu().numpy(), ctx.decode_acc(acc))
        for a in out[:5]:
            a.setflags(write=False)
        self.frames[key] = (out, ctx.last_kernel(), used, plan["reason"])
        return self.frames[key]

    def oracle_frame(self, name, ang, size, length=0):
        key = (name, ang, size, "oracle", length)
        if key not in self.frames:
            O = self.oracle
            sp = _scene(name)
            O.lib().ro_set_length_mode(length)
            try:
                sc = O.OracleScene(preset=sp if isinstance(sp, int) else None, accel="BVH", spheres=None if isinstance(sp, int) else sp)
                sc.set_angles(*ang)
                bufs = sc.render(*size)
                rgba = O.shade("iteration-heatmap", *bufs, *size)
            finally:
                O.lib().ro_set_length_mode(0)
            sdf, it = bufs[2].astype(np.int64), bufs[3].astype(np.int64)
            diag = {"total_sdf": int(sdf.sum()), "total_iters": int(it.sum()), "max_sdf": int(sdf.max()), "min_sdf": int(sdf.min())}
            self.frames[key] = bufs + (rgba, diag)
        return self.frames[key]


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


def check(renders, name, ang, size, length=0, taken=True, reason=0):
    """The frame with the rule against the frame without it, without in-round steps, and the CPU oracle's."""
    got, kernel, used, why = renders.gpu(name, ang, size, length=length)
    assert V2_AOT in kernel and V2_RTC not in kernel, kernel
    assert (used, why) == (taken, reason), "%s: the launch %s the rule (reason %d)" % (name, "applied" if used else "did not apply", why)
    what = "%s camera %s %dx%d length %d" % ((name, ang) + size + (length,))
    want, kernel, used, why = renders.gpu(name, ang, size, length=length, runner_up=0)
    assert V2_AOT in kernel and not used and why == 1, (kernel, used, why)
    same(got, want, what + ": against runner_up 0")
    want, kernel, used, why = renders.gpu(name, ang, size, length=length, multi_step=0)
    assert V2_AOT in kernel and not used and why == 2, (kernel, used, why)  # no in-round steps: no step-box table, no cell table
    same(got, want, what + ": against multi_step 0")
    same(got, renders.oracle_frame(name, ang, size, length), what + ": against the oracle")
    return got


@pytest.mark.parametrize("length", [0, 1], ids=lambda v: "length%d" % v)
@pytest.mark.parametrize("name", ["dense", "grid9", "around_camera"])
def test_sphere_grids(renders, name, length):
    check(renders, name, GOLDEN, SIZES[0], length)
    check(renders, name, ROTATED, SIZES[1], length)
    if name == "dense":
        check(renders, name, ROTATED, SIZES[0], length)
        check(renders, name, GOLDEN, SIZES[1], length)


@pytest.mark.parametrize("length", [0, 1], ids=lambda v: "length%d" % v)
@pytest.mark.parametrize("name", ["two_equal", "two_symmetric", "four_equal"])
def test_few_equal_spheres(renders, name, length):
    got = check(renders, name, GOLDEN, SIZES[0], length)
    assert got[3].max() >= 3  # rays that march
    check(renders, name, ROTATED, SIZES[1], length)


@pytest.mark.parametrize("length", [0, 1], ids=lambda v: "length%d" % v)
@pytest.mark.parametrize("name", ["one", "three_unequal"])
def test_scenes_without_one_radius_report_the_rule_as_not_taken(renders, name, length):
    check(renders, name, GOLDEN, SIZES[0], length, taken=False, reason=3)
    check(renders, name, ROTATED, SIZES[1], length, taken=False, reason=3)


@pytest.mark.parametrize("length", [0, 1], ids=lambda v: "length%d" % v)
def test_without_the_cell_table_the_rule_is_not_taken(renders, length):
    for name, ang, size in (("dense", GOLDEN, SIZES[0]), ("four_equal", ROTATED, SIZES[1])):
        got, kernel, used, why = renders.gpu(name, ang, size, length=length, cell_tab=0)
        assert V2_AOT in kernel and not used and why == 2, (kernel, used, why)
        want = renders.gpu(name, ang, size, length=length)
        assert want[2]
        same(got, want[0], "%s: cell_tab 0 against the rule" % name)


@pytest.mark.parametrize("length,size", [(0, SIZES[0]), (1, SIZES[1])], ids=["length0-160x90", "length1-96x54"])
def test_run_time_compiled_wave_loop(renders, length, size):
    """The copy of the wave loop compiled with the launch constants as literals, `runner_up` among them: it must be the kernel
    that ran (accepted, not refused for spills), and have applied the rule."""
    got, kernel, used, why = renders.gpu("dense", ROTATED, size, launches=3, specialise_v2_after=1, length=length)
    assert V2_RTC in kernel, kernel
    assert used and why == 0
    want, kernel, used, _ = renders.gpu("dense", ROTATED, size, length=length, runner_up=0)
    assert V2_RTC not in kernel and not used
    same(got, want, "compiled, runner_up 1: against the library's kernel with runner_up 0")
    same(got, renders.gpu("dense", ROTATED, size, length=length, multi_step=0)[0], "compiled, runner_up 1: against multi_step 0")
    same(got, renders.oracle_frame("dense", ROTATED, size, length), "compiled, runner_up 1: against the oracle")


@pytest.mark.parametrize("name", ["grid9", "two_equal", "two_symmetric", "four_equal"])
def test_run_time_compiled_wave_loop_small_scenes(renders, name):
    """The compiled copy with the constants of the small scenes as literals: no runner-up's bound behind k2 (two spheres: lb3
    infinite), a finite one (four), the preset grid; against the library's kernel without the rule and the oracle."""
    got, kernel, used, why = renders.gpu(name, GOLDEN, SIZES[1], launches=3, specialise_v2_after=1)
    assert V2_RTC in kernel, kernel
    assert used and why == 0
    want, kernel, used, _ = renders.gpu(name, GOLDEN, SIZES[1], runner_up=0)
    assert V2_RTC not in kernel and not used
    same(got, want, "%s compiled, runner_up 1: against the library's kernel with runner_up 0" % name)
    same(got, renders.oracle_frame(name, GOLDEN, SIZES[1]), "%s compiled, runner_up 1: against the oracle" % name)
