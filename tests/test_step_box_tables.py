"""The step-box tables of BVH sphere scenes (rm_scene_host.cpp build_step_box; scene array `step_tab`), on the CPU.

The in-round march steps of the v2 wave loop (rm_render_v2.hip, section M, option `step_box`) take a step when the new point lies
in the same cell of the per-axis thresholds as the round's point.  The thresholds are lo[k] and nextup(hi[k]) of every non-empty
leaf box and of the root; the cells are half-open, [T_i, T_i+1).  Checked here, from the table as rm_debug_scene_table returns it:

 * a numpy restatement of the kernel's look-up (bin byte, then the walk up) finds, for 10^4 seeded points in and around the root
   box and for every face coordinate, its nextup and its nextdown, the bracket a brute-force search over the leaf boxes finds;
 * two points of one bracket cell have the same binary32 `box_margin >= 0` membership in every leaf and in the root;
 * which scenes have a table, and what the launcher decides (rm_debug_step_box), without a device.
"""
import numpy as np
import pytest

F = np.float32
INF = F(np.inf)


def _up(v):
    return np.nextafter(F(v), INF, dtype=F)


def _down(v):
    return np.nextafter(F(v), -INF, dtype=F)


def _lattice(radii_seed=None):
    a = np.linspace(-1.2, 1.2, 5)
    g = np.array([[x, y, z] for z in a for y in a for x in a])
    r = np.full(125, 0.15) if radii_seed is None else np.random.default_rng(radii_seed).uniform(0.08, 0.3, 125)
    return g.astype(F), r


def _nine():
    g = np.array([[x, y, 0.0] for y in (-0.9, 0.0, 0.9) for x in (-0.9, 0.0, 0.9)], F)
    return g, np.linspace(0.22, 0.47, 9)


def _close_faces():  # two spheres whose faces differ by 1e-4 on x: several thresholds in one look-up bin
    g, r = _nine()
    g = np.concatenate([g, np.array([[0.0, 1.9, 0.3], [1e-4, -1.9, 0.3]], F)])
    return g, np.concatenate([r, [0.3, 0.3]])


def _tiny_face():  # a sphere at the origin whose padded box (centre -+ 1.5 r) has faces at -+1e-38
    g, r = _nine()
    g[4] = (0.0, 0.0, 0.0)
    r = r.copy()
    r[4] = 1e-38 / 1.5
    return g, r


SCENES = {
    "preset2": None, "preset3": None, "nine": _nine, "close_faces": _close_faces, "lattice_uniform": _lattice,
    "lattice_random": lambda: _lattice(8), "tiny_face": _tiny_face,
}
WITH_TABLE = ("preset2", "preset3", "nine", "close_faces", "lattice_uniform")
WITHOUT_TABLE = ("lattice_random", "tiny_face")


def _load(ctx, name):
    if name.startswith("preset"):
        ctx.scene_from_preset(int(name[6:]), 2)
    else:
        c, r = SCENES[name]()
        ctx.scene_from_spheres(c, r, 2)


def _boxes(ctx):
    """(lo, hi) of the root and of every non-empty leaf, float32 [m, 3]: the boxes the point-query lists are built from."""
    nodes = ctx.scene_table("bvh", from_device=False).reshape(-1, 32)
    lo, hi = nodes[:, 0:12].copy().view("<f4"), nodes[:, 16:28].copy().view("<f4")
    leaf = nodes[:, 28:32].copy().view("<i4").reshape(-1)
    keep = (leaf >= 0) & ((leaf & 0xFF) != 0)
    keep[0] = True
    return lo[keep], hi[keep], lo[0], hi[0]


def _thresholds(lo, hi, axis):
    return np.unique(np.concatenate([lo[:, axis], np.nextafter(hi[:, axis], INF, dtype=F)]))


class Table:
    def __init__(self, rm, ctx):
        from cpu_raymarcher_amd import _native as N
        self.words = ctx.scene_table("step_tab", from_device=False)
        self.bins = N.STEP_BOX_BINS
        self.stride = self.words.size // 3
        self.lo, self.hi, self.root_lo, self.root_hi = _boxes(ctx)

    def axis(self, k):
        w = self.words[k * self.stride:(k + 1) * self.stride]
        return w[:self.bins // 4].copy().view(np.uint8), w[self.bins // 4:].copy().view("<f4")

    def bracket(self, x, k):
        """The kernel's look-up in float32 arithmetic: (lo, hi, walk steps) per element of x."""
        bins, T = self.axis(k)
        ext = float(self.root_hi[k]) - float(self.root_lo[k])
        inv = F(self.bins / ext) if ext > 0 else F(0)
        g = (x - self.root_lo[k]).astype(F) * inv
        b = np.clip(np.trunc(g.astype(np.float64)), 0, self.bins - 1).astype(np.int64)
        last = self.stride - self.bins // 4 - 2
        i = np.minimum(bins[b].astype(np.int64), last)
        steps = np.zeros(len(x), np.int64)
        while True:
            more = (T[i + 1] <= x) & (i < last)
            if not more.any():
                break
            i += more
            steps += more
        return T[i], T[i + 1], steps


def _brute(th, x):
    """[T_i, T_i+1) around every x from the sorted distinct thresholds: -inf below the first, +inf above the last."""
    i = np.searchsorted(th, x, side="right")
    ext = np.concatenate([[-INF], th, [INF]]).astype(F)
    return ext[i], ext[i + 1]


def _member(lo, hi, p):
    """box_margin(lo, hi, p) >= 0 in binary32 for every box [m] and point [n, 3] -> bool [n, m]."""
    a = (p[:, None, :] - lo[None, :, :]).astype(F).min(axis=2)
    b = (hi[None, :, :] - p[:, None, :]).astype(F).min(axis=2)
    return np.minimum(a, b) >= 0


@pytest.fixture(scope="module")
def ctx(rm):
    c = rm.Context(None)
    yield c
    c.close()


@pytest.mark.parametrize("name", WITH_TABLE)
def test_lookup_finds_the_bracket_of_a_brute_force_search(rm, ctx, name):
    from cpu_raymarcher_amd import _native as N
    _load(ctx, name)
    t = Table(rm, ctx)
    assert t.words.size > 0 and t.words.size % 3 == 0
    rng = np.random.default_rng(21)
    for k in range(3):
        th = _thresholds(t.lo, t.hi, k)
        assert len(th) <= N.STEP_BOX_CAP
        bins, T = t.axis(k)
        assert T[0] == -INF and np.array_equal(T[1:1 + len(th)], th) and np.all(T[1 + len(th):] == INF) and len(T) >= len(th) + 2
        ext = float(t.root_hi[k] - t.root_lo[k])
        faces = np.concatenate([t.lo[:, k], t.hi[:, k]])
        edge = np.concatenate([faces, np.nextafter(faces, INF, dtype=F), np.nextafter(faces, -INF, dtype=F), th, np.nextafter(th, -INF, dtype=F)])
        x = np.concatenate([rng.uniform(t.root_lo[k] - 0.1 * ext, t.root_hi[k] + 0.1 * ext, 10000).astype(F), edge.astype(F)])
        lo, hi, steps = t.bracket(x, k)
        want_lo, want_hi = _brute(th, x)
        assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (name, k)
        assert np.all((lo <= x) & (x < hi))
        inside = (x >= t.root_lo[k]) & (x <= t.root_hi[k])
        if name == "close_faces" and k == 0:
            assert steps[inside].max() >= 2  # the two faces 1e-4 apart share a bin: the walk really walks
        elif name == "preset3":
            assert steps[inside].max() <= 1  # thresholds 0.15 apart, bins 0.089 wide


@pytest.mark.parametrize("name", WITH_TABLE)
def test_points_of_one_cell_have_the_same_leaves(rm, ctx, name):
    _load(ctx, name)
    t = Table(rm, ctx)
    rng = np.random.default_rng(22)
    n = 4000
    p, q = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for k in range(3):
        th = _thresholds(t.lo, t.hi, k)
        ext = float(t.root_hi[k] - t.root_lo[k])
        cells = np.concatenate([[F(t.root_lo[k] - 0.2 * ext)], th, [F(t.root_hi[k] + 0.2 * ext)]]).astype(F)
        i = rng.integers(0, len(cells) - 1, n)
        a, b = cells[i], np.nextafter(cells[i + 1], -INF, dtype=F)  # the cell as a closed binary32 interval
        u = rng.uniform(0, 1, (2, n))
        pk = np.clip((a + u[0] * (b.astype(np.float64) - a)).astype(F), a, b)
        qk = np.clip((a + u[1] * (b.astype(np.float64) - a)).astype(F), a, b)
        ends = rng.integers(0, 4, n)  # a quarter of the pairs: one point on the cell's first value, the other on its last
        pk[ends == 0], qk[ends == 0] = a[ends == 0], b[ends == 0]
        p[:, k], q[:, k] = pk, qk
        lo_p, hi_p, _ = t.bracket(pk, k)
        lo_q, hi_q, _ = t.bracket(qk, k)
        assert np.array_equal(lo_p, lo_q) and np.array_equal(hi_p, hi_q)  # one cell by the table's own look-up too
    mp, mq = _member(t.lo, t.hi, p), _member(t.lo, t.hi, q)
    assert np.array_equal(mp, mq), (name, int((mp != mq).sum()))
    assert mp[:, 0].any() and not mp[:, 0].all() and mp[:, 1:].any()  # the pairs cover inside and outside of the root, and leaves


def test_which_scenes_have_a_table_and_what_the_launcher_decides(rm, ctx):
    from cpu_raymarcher_amd import _native as N
    ctx.set_option("kernel", 2)
    try:
        for name in WITH_TABLE + WITHOUT_TABLE:
            _load(ctx, name)
            words = ctx.scene_table("step_tab", from_device=False)
            lo, hi, _, _ = _boxes(ctx)
            most = max(len(_thresholds(lo, hi, k)) for k in range(3))
            s = ctx.step_box()
            if name in WITH_TABLE:
                assert words.size == 3 * (N.STEP_BOX_BINS // 4 + most + 2) and s["table_bytes"] == 4 * words.size
                assert s["planned"] and s["reason"] == 0, (name, s)
            else:
                assert words.size == 0 and s["table_bytes"] == 0
                assert not s["planned"] and s["reason"] == 2, (name, s)
            assert not s["last"]  # nothing was launched
        _load(ctx, "lattice_random")
        lo, hi, _, _ = _boxes(ctx)
        assert max(len(_thresholds(lo, hi, k)) for k in range(3)) > N.STEP_BOX_CAP  # that is why
        _load(ctx, "tiny_face")
        lo, hi, _, _ = _boxes(ctx)
        faces = np.abs(np.concatenate([lo.ravel(), hi.ravel()]))
        assert ((faces > 0) & (faces < 1e-30)).any()
        # the Dense Sphere Grid: the table rides in the LDS the launch had left -- the hit lists keep their 13 entries
        _load(ctx, "preset3")
        s = ctx.step_box()
        assert s["planned"] and s["list_cap"] == s["list_cap_without"] == 13 and s["table_bytes"] == 240, s
        for key in ("step_box", "multi_step"):
            ctx.set_option(key, 0)
            s = ctx.step_box()
            assert not s["planned"] and s["reason"] == 1, (key, s)
            ctx.set_option(key, 1)
        ctx.set_option("kernel", 1)
        assert ctx.step_box()["reason"] == 1
        ctx.set_option("kernel", 2)
        # no room: a budget (lds_kb) and a hit-list capacity that the scene's tables just reach without the table
        found = None
        for kb in range(16, 65):
            for cap in range(1, 13):
                ctx.set_option("lds_kb", kb)
                ctx.set_option("list_cap", cap)
                s = ctx.step_box()
                if s["reason"] == 3:
                    found = found or (kb, cap)
                    assert not s["planned"] and s["list_cap"] == s["list_cap_without"] == cap, s
                else:
                    assert s["planned"] and s["reason"] == 0, (kb, cap, s)
        assert found is not None
    finally:
        for key, v in (("kernel", 0), ("lds_kb", 0), ("list_cap", 32), ("step_box", 1), ("multi_step", 1)):
            ctx.set_option(key, v)


def test_an_edit_leaves_the_table_of_an_upload(rm, ctx):
    c, r = _nine()
    ctx.scene_from_spheres(c, r, 2)
    before = ctx.scene_table("step_tab", from_device=False).copy()
    ctx.edit_spheres([("set", 4, (0.1, 0.05, 0.3), 0.4), ("insert", 9, (1.5, 1.5, -0.5), 0.2)])
    got = ctx.scene_table("step_tab", from_device=False).copy()
    c2, r2 = c.copy(), list(r)
    c2[4], r2[4] = (0.1, 0.05, 0.3), 0.4
    c2 = np.concatenate([c2, np.array([[1.5, 1.5, -0.5]], F)])
    r2.append(0.2)
    ctx.scene_from_spheres(c2, r2, 2)
    want = ctx.scene_table("step_tab", from_device=False)
    assert got.size and np.array_equal(got, want) and not np.array_equal(got, before)
