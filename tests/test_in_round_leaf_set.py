"""In-round march steps of the v2 wave loop (rm_render_v2.hip, section M) under the exact leaf-set test: a lane goes on
stepping inside a round for as long as the leaves that contain the new point -- looked up in the new point's own cell --
are the leaves that contained the round's point.  The steps are the ordinary path's steps or they are a bug, so every
check here is byte equality: the five buffers (depth, normal, SDF evaluations, iterations, shaded RGBA) and the four fused
diagnostics of the wave loop with `multi_step` 1 against (a) the same loop with `multi_step` 0, (b) the one-ray-per-lane
kernel (`kernel` 1) and (c) the CPU oracle.

Frames are 200 x 136 (partial tiles in both directions, several workgroups) and 640 x 360."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL, LARGE = (200, 136), (640, 360)
NAMES = ("depth", "normal", "sdf", "iters", "rgba", "diagnostics")
DEFAULTS = dict(kernel=2, multi_step=1, specialise=1, specialise_v2_after=0, list_cap=32, lds_kb=0, length=0, uniform=1, rel=1)
V2_AOT = "render_kernel_v2<"
V2_RTC = "[launch constants compiled in]"


def _dense(oracle):
    c, r = oracle.OracleScene(preset=3, accel="BVH").spheres()
    return np.concatenate([c.astype(np.float64), r.reshape(-1, 1)], axis=1).astype(np.float32)


def _scene(oracle, name):
    """float32 [n, 4] spheres of a named scene, or None for the Dense Sphere Grid preset itself."""
    rng = np.random.default_rng(8)
    if name == "dense":  # 64 leaves of at most two spheres, abutting: as many leaves at p2 as at q, but other leaves
        return None
    if name == "nine":  # nine spheres in a plane, radii all different (UR = false; a small tree: the origin-relative build)
        g = np.array([[x, y, 0.0] for y in (-0.9, 0.0, 0.9) for x in (-0.9, 0.0, 0.9)])
        return np.concatenate([g, np.linspace(0.22, 0.47, 9).reshape(-1, 1)], axis=1).astype(np.float32)
    if name == "lattice125":  # 5 x 5 x 5, radii from touching to well apart
        a = np.linspace(-1.2, 1.2, 5)
        g = np.array([[x, y, z] for z in a for y in a for x in a])
        return np.concatenate([g, rng.uniform(0.08, 0.3, (125, 1))], axis=1).astype(np.float32)
    if name == "inverted":  # one negative radius: that sphere's box has lo > hi and contains nothing
        sp = _scene(oracle, "nine")
        sp[4, 3] = -0.3
        return sp
    if name == "skim":  # tall and thin: most rays run along the long faces of the root box, in and out of it within an ulp
        y = np.linspace(-2.4, 2.4, 25)
        g = np.stack([0.05 * np.sin(7.0 * y), y, 0.05 * np.cos(5.0 * y)], axis=1)
        return np.concatenate([g, np.full((25, 1), 0.11) + 0.02 * np.cos(3.0 * y).reshape(-1, 1)], axis=1).astype(np.float32)
    if name == "inside":  # the dense grid moved around the camera: rays start between its spheres
        sp = _dense(oracle)
        _, org = oracle.OracleScene(preset=3, accel="BVH").camera()
        c = sp[:, :3].astype(np.float64)
        mid = 0.5 * (c.min(axis=0) + c.max(axis=0))
        pitch = np.sort(np.unique(np.round(c[:, 0], 4)))
        step = float(pitch[1] - pitch[0]) if len(pitch) > 1 else 1.0
        sp[:, :3] = (c - mid + org.astype(np.float64) + step * np.array([0.5, 0.43, 0.37])).astype(np.float32)
        return sp
    raise KeyError(name)


class Renders:
    """One context for the module; the oracle's frames are computed once per (scene, size, camera, length) and shared."""

    def __init__(self, rm, oracle):
        import torch
        self.rm, self.oracle, self.torch = rm, oracle, torch
        self.ctx = rm.Context(0)
        self.dev = torch.device("cuda:0")
        self.want = {}
        self.spheres = {}

    def scene_spheres(self, name):
        if name not in self.spheres:
            self.spheres[name] = _scene(self.oracle, name)
        return self.spheres[name]

    def gpu(self, name, size, ang, **opts):
        """(depth, normal, sdf, iters, rgba, diagnostics) of one frame, and the kernel that rendered it."""
        torch, ctx = self.torch, self.ctx
        launches = 1 + int(opts.pop("launches_before", 0))  # (the run-time compiled kernel takes over after some launches)
        for k, v in dict(DEFAULTS, **opts).items():
            ctx.set_option(k, v)
        sc = self.rm.Scene("BVH", ctx=ctx)
        sp = self.scene_spheres(name)
        if sp is None:
            sc.loadPreset(3)
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
        for _ in range(launches):
            tracer.runRaymarcher(sc, d, nr, s16, i16, W, H, 0.0, shadedBuffer=rgba, shader="iteration-heatmap", diagnostics=acc)
            torch.cuda.synchronize()
        diag = ctx.decode_acc(acc)
        out = (d.cpu().numpy(), nr.cpu().numpy(), s16.cpu().numpy().view(np.uint16), i16.cpu().numpy().view(np.uint16),
               rgba.cpu().numpy(), diag)
        return out, ctx.last_kernel()

    def cpu(self, name, size, ang, length=0):
        key = (name, size, ang, length)
        if key not in self.want:
            O = self.oracle
            sp = self.scene_spheres(name)
            O.lib().ro_set_length_mode(length)
            try:
                sc = O.OracleScene(preset=3 if sp is None else None, accel="BVH", spheres=sp)
                sc.set_angles(*ang)
                W, H = size
                bufs = sc.render(W, H)
                rgba = O.shade("iteration-heatmap", *bufs, W, H)
            finally:
                O.lib().ro_set_length_mode(0)
            sdf, it = bufs[2].astype(np.int64), bufs[3].astype(np.int64)
            diag = {"total_sdf": int(sdf.sum()), "total_iters": int(it.sum()), "max_sdf": int(sdf.max()), "min_sdf": int(sdf.min())}
            self.want[key] = bufs + (rgba, diag)
            for a in self.want[key][:5]:
                a.setflags(write=False)
        return self.want[key]


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


def check(renders, name, size, ang, v2=V2_AOT, length=0, **opts):
    """The wave loop with in-round steps against the three references; returns its frame."""
    got, kernel = renders.gpu(name, size, ang, multi_step=1, length=length, **opts)
    assert v2 in kernel, kernel  # the wave loop rendered it (and the build the case names)
    if length:
        assert "[length=sqrt]" in kernel, kernel
    what = "%s %dx%d camera %s %s" % (name, size[0], size[1], ang, opts)
    ref_a, kernel_a = renders.gpu(name, size, ang, multi_step=0, length=length, **{k: v for k, v in opts.items() if k != "launches_before"})
    assert V2_AOT in kernel_a, kernel_a
    same(got, ref_a, what + ": against multi_step 0")
    ref_b, kernel_b = renders.gpu(name, size, ang, kernel=1, length=length)
    assert "v2" not in kernel_b, kernel_b
    same(got, ref_b, what + ": against the one-ray-per-lane kernel")
    same(got, renders.cpu(name, size, ang, length), what + ": against the oracle")
    return got


GOLDEN = (0.0, 0.0)
CAMERAS = [GOLDEN, (0.0, 0.3), (0.0, 0.785), (0.4, 0.3), (-0.4, 0.785)]


@pytest.mark.parametrize("ang", CAMERAS, ids=lambda a: "pitch%g-yaw%g" % a)
def test_dense_grid_equal_counts_other_leaf(renders, ang):
    """Abutting leaves of one or two spheres: a step from one leaf into the next finds as many leaves as before, and
    other ones -- the count alone must not let the run go on."""
    check(renders, "dense", SMALL, ang)


def test_dense_grid_and_lattice_at_640_by_360(renders):
    check(renders, "dense", LARGE, GOLDEN)
    check(renders, "lattice125", LARGE, (0.3, 0.7))


def test_camera_inside_the_lattice(renders):
    for ang in (GOLDEN, (0.4, 0.785)):
        check(renders, "inside", SMALL, ang)


@pytest.mark.parametrize("name", ["nine", "lattice125", "inverted", "skim"])
def test_non_uniform_radii_inverted_box_and_skimming_rays(renders, name):
    for ang in (GOLDEN, (0.4, 0.3), (1.2, 0.785)):
        check(renders, name, SMALL, ang)
    check(renders, name, SMALL, (-0.4, 0.785), uniform=0, rel=0)


@pytest.mark.parametrize("opts", [dict(list_cap=2), dict(list_cap=16), dict(lds_kb=16), dict(lds_kb=32), dict(lds_kb=40, list_cap=2)],
                         ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
def test_shrunk_hit_lists(renders, opts):
    check(renders, "dense", SMALL, (0.4, 0.3), **opts)
    check(renders, "lattice125", SMALL, (0.0, 0.785), **opts)


@pytest.mark.parametrize("name,ang", [("dense", GOLDEN), ("dense", (-0.4, 0.785)), ("lattice125", (0.4, 0.3)), ("inside", GOLDEN)])
def test_length_sqrt_build(renders, name, ang):
    check(renders, name, SMALL, ang, length=1)


@pytest.mark.parametrize("name,length", [("dense", 0), ("lattice125", 0), ("dense", 1)])
def test_run_time_compiled_wave_loop(renders, name, length):
    """The copy of the wave loop compiled at run time with the launch constants as literals, after `specialise_v2_after`
    launches: it must be the kernel that ran, and its bytes those of the ahead-of-time kernel and of the references."""
    ang = (0.4, 0.3)
    aot = check(renders, name, SMALL, ang, specialise=0, length=length)
    rtc = check(renders, name, SMALL, ang, v2=V2_RTC, length=length, specialise_v2_after=1, launches_before=2)
    same(rtc, aot, "compiled against ahead-of-time")


def _ulps(v, k):
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return v


@pytest.mark.parametrize("name", ["dense", "lattice125", "inverted"])
def test_point_queries_beside_leaf_and_cell_faces(renders, oracle, name):
    """Section M repeats bvh_distance_wave's own look-up at the new point.  That look-up, on points one and two ulps either
    side of every leaf-box face and of every cell face of the leaf grid (and on the faces), must give the oracle's
    getDistance: value and evaluation count."""
    ctx = renders.ctx
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    sc = renders.rm.Scene("BVH", ctx=ctx)
    sp = renders.scene_spheres(name)
    if sp is None:
        sc.loadPreset(3)
    else:
        sc.loadSpheres(sp[:, :3], sp[:, 3])
    nodes = ctx.scene_table("bvh").reshape(-1, 32)
    lo, hi = nodes[:, 0:12].copy().view("<f4"), nodes[:, 16:28].copy().view("<f4")
    leaf = nodes[:, 28:32].copy().view("<i4").reshape(-1)
    info = ctx.scene_info()
    rmin, rmax = np.array(info["root_min"], np.float32), np.array(info["root_max"], np.float32)
    g = max(2, min(int(np.ceil(np.cbrt(float(info["bvh_leaves"])) * 3.0)), 32))  # the leaf grid's cells per axis
    rng = np.random.default_rng(5)
    pts = []
    for i in np.nonzero(leaf >= 0)[0]:
        if not np.all(lo[i] <= hi[i]):
            continue
        for axis in range(3):
            for face in (lo[i, axis], hi[i, axis]):
                for k in (-2, -1, 0, 1, 2):
                    for _ in range(2):
                        p = rng.uniform(lo[i], hi[i]).astype(np.float32)
                        p[axis] = _ulps(face, k)
                        pts.append(p)
    for axis in range(3):
        ext = float(rmax[axis]) - float(rmin[axis])
        inv = np.float32(g / ext)
        for c in range(g + 1):
            for face in (np.float32(float(rmin[axis]) + c / float(inv)), np.float32(rmin[axis] + np.float32(c) / inv)):
                for k in (-2, -1, 0, 1, 2):
                    for _ in range(6):
                        p = rng.uniform(rmin, rmax).astype(np.float32)
                        p[axis] = _ulps(face, k)
                        pts.append(p)
    pts = np.array(pts, np.float32)
    assert len(pts) > 1000
    d, c = ctx.wave_distance(pts)
    osc = oracle.OracleScene(preset=3 if sp is None else None, accel="BVH", spheres=sp)
    want = [osc.distance(p) for p in pts]
    assert np.array_equal(d, np.array([w[0] for w in want]))
    assert np.array_equal(c, np.array([w[1] for w in want], np.uint32))
