"""Option `exact` on the GPU (include/rm_raymarch.h, "the exact field").  The oracle is the existing code: for every case a second
context holds the same scene uploaded with acceleration None and exact = 0, and an exact query of the first context -- whatever
its acceleration structure -- must return that context's bytes (count excepted: under a tree it is the evaluations made).  There
are no tolerances: every comparison is of raw bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

NONE, OCTREE, BVH = 0, 1, 2
N_POINTS = 4099  # not a multiple of 64
LIST_CAP = 1024  # RM_EXACT_LIST_CAP of csrc/rm_kernels.hip: ids a tile's candidate list holds


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same(a, b):
    return (a is None and b is None) or np.array_equal(bits(a), bits(b))


def grid_spheres():
    """The centres of preset 3: 5 x 5 x 5 spheres of radius 0.15, 0.6 apart, z fastest (binary32 values, widened)."""
    return np.array([[x * 0.6 - 1.2, y * 0.6 - 1.2, z * 0.6 - 1.2] for x in range(5) for y in range(5) for z in range(5)], np.float32).astype(np.float64)


def sphere_list(n, seed):
    from cpu_raymarcher_amd import synthetic as S
    s = S.synthetic_spheres(n, seed)
    return s[:, :3].astype(np.float32), s[:, 3].copy()


def mixed(rm, scaled=False):
    from cpu_raymarcher_amd import synthetic as S
    t = S.mixed_prims_as_triples(S.synthetic_mixed_prims(12), rm.make_transform)
    if scaled:
        kind, m, par = t[4]
        t[4] = (kind, rm.scale_transform(m, 1.0, 1.5, 0.75), par)
    return t


# name -> (loader(ctx, accel), accelerations, the mode rm_debug_exact_tree reports per acceleration, objects, time)
def scene_table(rm):
    c300, r300 = sphere_list(300, 300)
    few_c, few_r = np.float32([[0.25, 0, 0], [-0.75, 0.5, 0], [0, -1, 0.5]]), np.array([0.5, 0.25, 0.125])
    table = {
        "grid": (lambda ctx, a: ctx.scene_from_preset(3, a), (BVH, OCTREE, NONE), {BVH: 1, OCTREE: 2, NONE: 2}, 125, 0.0),
        "s300": (lambda ctx, a: ctx.scene_from_spheres(c300, r300, a), (OCTREE,), {OCTREE: 2}, 300, 0.0),
        "s0": (lambda ctx, a: ctx.scene_from_spheres(few_c[:0], few_r[:0], a), (OCTREE, BVH), {OCTREE: 0, BVH: 0}, 0, 0.0),
        "prims": (lambda ctx, a: ctx.scene_from_prims(mixed(rm), a), (BVH, OCTREE), {BVH: 1, OCTREE: 2}, 12, 0.0),
        "scaled": (lambda ctx, a: ctx.scene_from_prims(mixed(rm, True), a), (BVH, OCTREE), {BVH: 0, OCTREE: 0}, 12, 0.0),
        "smooth": (lambda ctx, a: ctx.scene_from_preset(10, a), (OCTREE,), {OCTREE: 0}, None, 0.0),
        "animated": (lambda ctx, a: ctx.scene_from_preset(12, a), (OCTREE,), {OCTREE: 0}, None, 0.7),
    }
    for k in (1, 2, 3):
        table["s%d" % k] = (lambda ctx, a, k=k: ctx.scene_from_spheres(few_c[:k], few_r[:k], a), (OCTREE, BVH), {OCTREE: 2, BVH: 1}, k, 0.0)
    return table


CASES = [("grid", BVH), ("grid", OCTREE), ("grid", NONE), ("s300", OCTREE), ("s1", OCTREE), ("s2", BVH), ("s3", OCTREE), ("s3", BVH), ("s0", OCTREE),
         ("s0", BVH), ("prims", BVH), ("prims", OCTREE), ("scaled", BVH), ("scaled", OCTREE), ("smooth", OCTREE), ("animated", OCTREE)]


def make_points():
    """4 099 points: uniform ones, 64 outside the octree's cube, sphere centres, points on the spheres and points at the same
    distance from four or eight spheres of the grid (the tie rule: the lowest index).  The ties are exact: f32(0.6) is twice
    f32(0.3), so (+-0.3f, +-0.3f, z) differs from the centres of four neighbouring spheres by the same three magnitudes."""
    rng = np.random.default_rng(11)
    c300, r300 = sphere_list(300, 300)
    g = grid_spheres()
    far = rng.uniform(-2.5, 2.5, (64, 3))
    far[np.arange(64), rng.integers(0, 3, 64)] = rng.choice([-1.0, 1.0], 64) * rng.uniform(10.5, 14.0, 64)
    on_surface = np.concatenate([c300.astype(np.float64) + r300[:, None] * np.float64([1, 0, 0]), g + 0.15 * np.float64([0, 0, 1])])
    h = float(np.float32(0.3))
    ties = np.array([(sx * h, sy * h, z) for sx in (-1, 1) for sy in (-1, 1) for z in rng.uniform(-1.5, 1.5, 23)] +
                    [(sx * h, sy * h, sz * h) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    d2 = ((ties[:, None, :] - g[None, :, :]) ** 2).sum(axis=2)
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 4).all()
    fixed = np.concatenate([far, c300, g, on_surface, ties])
    pts = np.concatenate([fixed, rng.uniform(-2.5, 2.5, (N_POINTS - len(fixed), 3))]).astype(np.float32)
    assert len(pts) == N_POINTS and N_POINTS % 64
    return pts


@pytest.fixture(scope="module")
def points():
    return make_points()


@pytest.fixture(scope="module")
def pair(rm):
    """(ctx, ref): the context under test and the acceleration-None oracle, exact = 0 there."""
    ctx, ref = rm.Context(0), rm.Context(0)
    yield ctx, ref
    ctx.close()
    ref.close()


def load(rm, pair, name, accel):
    ctx, ref = pair
    loader, _, modes, n_objects, time = scene_table(rm)[name]
    ctx.set_option("exact", 0)
    loader(ctx, accel)
    loader(ref, NONE)
    assert ref.get_option("exact") == 0
    assert ctx.exact_tree()["mode"] == modes[accel], (name, accel)
    if n_objects is None:
        n_objects = ref.scene_info()["n_prims"]
    return ctx, ref, modes[accel], n_objects, time


@pytest.mark.parametrize("name,accel", CASES)
def test_point_queries_equal_the_none_context(rm, pair, points, name, accel):
    import torch
    ctx, ref, mode, n_objects, time = load(rm, pair, name, accel)
    for snap, normal, iso in ((0, False, 0.0), (0, True, 0.05), (3, True, 0.0), (3, False, 0.05), (16, True, 0.0), (16, False, 0.05)):
        what = (name, accel, snap, normal, iso)
        want = ref.points(points, normal=normal, object=True, snap=snap, iso=iso, time=time)
        got = ctx.points(points, normal=normal, object=True, snap=snap, iso=iso, time=time, exact=True)
        assert "point_kernel<EXACT, " in ctx.last_kernel(), ctx.last_kernel()
        for field in ("position", "dist", "normal", "object", "steps"):
            assert same(getattr(got, field), getattr(want, field)), (what, field)
        # the None context counts every object at every evaluation: objects x evaluations of the lane
        if mode == 0:
            assert np.array_equal(got.count, want.count), what
        else:
            assert (got.count <= want.count).all(), what
        # the device entry, in place: d_position == d_points
        d_pts = torch.from_numpy(points).cuda()
        q = ctx._point_query(normal, snap, 1e-4, iso, time)
        ctx.set_option("exact", 1)
        try:
            dist, nrm, obj, steps, cnt = ctx._points_device(q, d_pts, d_pts, normal, True)
        finally:
            ctx.set_option("exact", 0)
        torch.cuda.synchronize()
        assert same(d_pts.cpu().numpy(), got.position) and same(dist.cpu().numpy(), got.dist) and same(obj.cpu().numpy(), got.object), what
        assert same(steps.cpu().numpy(), got.steps) and same(cnt.cpu().numpy(), got.count), what
        if normal:
            assert same(nrm.cpu().numpy(), got.normal), what
    assert ctx.get_option("exact") == 0


def test_an_exact_projection_moves_where_the_octree_field_is_flat(rm, pair, points):
    """The 300-sphere octree scene: in an empty leaf Scene.getDistance is a constant, its gradient (0, 0, 0), and a projection
    stops at once; the exact field has a gradient there, so every such point farther than tol from the surface steps."""
    ctx, ref, _, _, _ = load(rm, pair, "s300", OCTREE)
    tol = 1e-4
    at = ctx.points(points, normal=True, object=False, snap=0)
    # inside the cube, no primitive evaluated at the point or beside it, no gradient: the point and its offsets in empty leaves
    flat = (at.count == 0) & (np.abs(points).max(axis=1) <= 10.0) & (at.normal == 0).all(axis=1)
    far = np.abs(ref.points(points, normal=False, object=False).dist) > tol
    sel = flat & far
    print("points in flat empty leaves and off the surface:", int(sel.sum()))
    assert sel.sum() > 500
    plain = ctx.points(points, normal=True, object=False, snap=3, tol=tol)
    assert (plain.steps[sel] == 0).all()
    exact = ctx.points(points, normal=True, object=False, snap=3, tol=tol, exact=True)
    assert (exact.steps[sel] >= 1).all()


@pytest.mark.parametrize("name,accel", CASES)
def test_fields_equal_the_none_context(rm, pair, name, accel):
    ctx, ref, mode, n_objects, time = load(rm, pair, name, accel)
    lattice = dict(origin=(-2.4, -1.3, -0.9), du=(0.15, 0, 0.01), dv=(0.02, 0.16, -0.01), dw=(0, 0.03, 0.2), shape=(33, 17, 9), time=time)
    want, _ = ref.field(**lattice)
    got, count = ctx.field(exact=True, **lattice)
    assert "field_kernel<EXACT, " in ctx.last_kernel(), ctx.last_kernel()
    assert same(got, want), (name, accel)
    assert (count <= n_objects).all()
    if mode == 0:
        assert (count == n_objects).all()
    want32, _ = ref.field(dist32=True, count=False, **lattice)
    got32, _ = ctx.field(dist32=True, count=False, exact=True, **lattice)
    assert same(got32, want32), (name, accel)
    d, c = ctx.field(device=True, exact=True, **lattice)
    assert same(d.cpu().numpy(), want) and same(c.cpu().numpy(), count)
    # a slice: nw = 1
    want, _ = ref.field_slice("y", 0.3, 2.5, (37, 21), time=time)
    got, count = ctx.field_slice("y", 0.3, 2.5, (37, 21), time=time, exact=True)
    assert same(got, want) and (count <= n_objects).all()
    assert ctx.get_option("exact") == 0


def run_tiles(rm, ctx, lat, blocks):
    import torch
    N = rm._native
    k = blocks.n_kept
    tiles = torch.full((max(k, 1), 729), -7.0, dtype=torch.float64, device="cuda")
    N.check(ctx._h, N.lib().rm_scene_tiles_device(ctx._h, C.byref(lat), C.c_void_p(blocks.list.data_ptr()) if k else None, k,
                                                  C.c_void_p(tiles.data_ptr()) if k else None, None))
    torch.cuda.synchronize()
    return tiles.cpu().numpy()[:k]


def host_sparse(rm, ctx, lat, iso):
    """rm_scene_mesh_sparse: (vertices, quads, cells, edges, mesh info, sparse info)."""
    N = rm._native
    info, sinfo = N.rm_mesh_info(), N.rm_sparse_info()
    call = N.lib().rm_scene_mesh_sparse
    N.check(ctx._h, call(ctx._h, C.byref(lat), iso, 1.0, None, 0, None, 0, None, None, C.byref(info), C.byref(sinfo)))
    nv, nq = info.n_vertices, info.n_quads
    v, q = np.zeros((max(nv, 1), 3), np.float32), np.zeros((max(nq, 1), 4), np.uint32)
    ce, ed = np.zeros(max(nv, 1), np.int64), np.zeros(max(nq, 1), np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N.check(ctx._h, call(ctx._h, C.byref(lat), iso, 1.0, vp(v), nv, vp(q), nq, vp(ce), vp(ed), C.byref(info), C.byref(sinfo)))
    return v[:nv], q[:nq], ce[:nv], ed[:nq], bytes(info), bytes(sinfo)


@pytest.mark.parametrize("accel", [OCTREE, BVH])
@pytest.mark.parametrize("iso", [0.0, 0.05])
def test_meshes_and_tiles_equal_the_none_context(rm, pair, accel, iso):
    """Preset 3 over 27^3 points: four blocks per axis, the last one partial (two cells)."""
    ctx, ref, _, _, _ = load(rm, pair, "grid", accel)
    axes = ((-2.6, -2.6, -2.6), (0.2, 0, 0), (0, 0.2, 0), (0, 0, 0.2), (27, 27, 27))
    want = ref.mesh(*axes, iso=iso)
    got = ctx.mesh(*axes, iso=iso, exact=True)
    assert len(want[0]) > 0 and same(got[0], want[0]) and same(got[1], want[1])
    N = rm._native
    lat = rm.make_lattice(*axes)
    info_w, info_g = N.rm_mesh_info(), N.rm_mesh_info()
    N.check(ref._h, N.lib().rm_scene_mesh(ref._h, C.byref(lat), iso, None, 0, None, 0, C.byref(info_w)))
    ctx.set_option("exact", 1)
    try:
        N.check(ctx._h, N.lib().rm_scene_mesh(ctx._h, C.byref(lat), iso, None, 0, None, 0, C.byref(info_g)))
        assert bytes(info_g) == bytes(info_w)
        got_sparse = host_sparse(rm, ctx, lat, iso)
        blocks = ctx.sparse_blocks(*axes, iso=iso)
        tiles = run_tiles(rm, ctx, lat, blocks)
        assert "tiles_kernel<EXACT, 0>" in ctx.last_kernel()
    finally:
        ctx.set_option("exact", 0)
    want_sparse = host_sparse(rm, ref, lat, iso)
    for g, w in zip(got_sparse, want_sparse):
        assert same(np.frombuffer(g, np.uint8) if isinstance(g, bytes) else g, np.frombuffer(w, np.uint8) if isinstance(w, bytes) else w)
    ref_blocks = ref.sparse_blocks(*axes, iso=iso)
    assert same(blocks.list.cpu().numpy(), ref_blocks.list.cpu().numpy()) and blocks.dims == (4, 4, 4)
    want_tiles = run_tiles(rm, ref, lat, ref_blocks)
    assert np.isnan(want_tiles).any()  # the padding of the partial blocks
    assert same(tiles, want_tiles)
    # the Python mirror, with exact attributes
    w = ref.mesh_sparse(*axes, iso=iso, attributes=True, snap=2)
    g = ctx.mesh_sparse(*axes, iso=iso, attributes=True, snap=2, exact=True)
    assert all(same(a, b) for a, b in zip(g, w))


def test_a_tile_whose_candidate_list_overflows_and_one_without_a_candidate(rm, pair):
    """The list holds LIST_CAP = 1 024 ids.  2 000 spheres of radius 0.01 in a cube of side 0.4 around the origin, a lattice step
    of 0.5: a tile spans 4 units, so the tile around the origin (block 3, 3, 3: -2 .. 2) has all 2 000 leaves' boxes inside its own
    box -- every object is a candidate whatever U is, the list overflows and the workgroup takes the per-lane walk.  57 points per
    axis from -14 on: the corner tile (-14 .. -10) is more than 16 away from every sphere, so E = 10 on it and -- with
    U = 10 + 4 * 3 * 0.5 = 16 -- no leaf is a candidate.  The coarse pass is by-passed: every block's tile is asked for."""
    import torch
    ctx, ref = pair
    rng = np.random.default_rng(3)
    centers = rng.uniform(-0.2, 0.2, (2000, 3)).astype(np.float32)
    radii = np.full(2000, 0.01)
    assert len(radii) > LIST_CAP
    axes = ((-14, -14, -14), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 0.5), (57, 57, 57))
    lat = rm.make_lattice(*axes)
    n_blocks = 7 * 7 * 7
    from cpu_raymarcher_amd.context import SparseBlocks
    every = SparseBlocks(None, torch.arange(n_blocks, dtype=torch.int32, device="cuda"), None, n_blocks, (7, 7, 7))
    ref.scene_from_spheres(centers, radii, NONE)
    ref.set_option("exact", 0)
    want = run_tiles(rm, ref, lat, every)
    assert (want[0] == 10.0).all() and (want[(3 * 7 + 3) * 7 + 3] < 4.0).all()  # a corner tile; the tile around the origin
    for accel in (OCTREE, BVH):
        ctx.scene_from_spheres(centers, radii, accel)
        assert ctx.exact_tree()["mode"] == (2 if accel == OCTREE else 1)
        ctx.set_option("exact", 1)
        try:
            got = run_tiles(rm, ctx, lat, every)
        finally:
            ctx.set_option("exact", 0)
        assert same(got, want), accel


def test_an_edited_scene_answers_from_a_fresh_tree(rm, pair, points):
    ctx, ref = pair
    c, r = sphere_list(300, 300)
    ctx.set_option("exact", 0)
    ctx.scene_from_spheres(c, r, OCTREE)
    ref.scene_from_spheres(c, r, NONE)
    before = ctx.exact_tree()
    ctx.points(points[:256], exact=True)
    edits = [("set", 17, (0.1, 0.2, 0.3), 0.3), ("insert", 5, (2.0, 2.0, 2.0), 0.15), ("remove", 200), ("insert", 0, (-2.0, 2.0, 1.0), 0.2),
             ("insert", 0, (-2.0, -2.0, 1.0), 0.2)]
    ctx.edit_spheres(edits)
    ref.edit_spheres(edits)
    want = ref.points(points, snap=2)
    got = ctx.points(points, snap=2, exact=True)
    for field in ("position", "dist", "normal", "object", "steps"):
        assert same(getattr(got, field), getattr(want, field)), field
    after = ctx.exact_tree()
    assert after["mode"] == 2 and after != before  # 302 spheres now: another tree
    moved = np.float32([[0.1, 0.2, 0.3], [2.0, 2.0, 2.0]])
    assert (ctx.points(moved, exact=True).dist < 0).all()


@pytest.mark.parametrize("name,accel", [("grid", BVH), ("s300", OCTREE)])
def test_without_the_option_nothing_changes(rm, points, name, accel):
    """Points, field, tiles and rm_last_kernel with exact = 0 after the option has been used equal those of a fresh context
    on which it was never set."""
    loader = scene_table(rm)[name][0]
    axes = ((-2.6, -2.6, -2.6), (0.2, 0, 0), (0, 0.2, 0), (0, 0, 0.2), (27, 27, 27))
    lat = rm.make_lattice(*axes)

    def answers(ctx):
        out = []
        p = ctx.points(points, snap=3)
        out += [bits(x) for x in p] + [ctx.last_kernel()]
        d, c = ctx.field(*axes[:4], shape=axes[4])
        out += [bits(d), bits(c), ctx.last_kernel()]
        out += [bits(run_tiles(rm, ctx, lat, ctx.sparse_blocks(*axes))), ctx.last_kernel()]
        return out

    fresh = rm.Context(0)
    loader(fresh, accel)
    want = answers(fresh)
    fresh.close()
    used = rm.Context(0)
    loader(used, accel)
    used.points(points, snap=3, exact=True)
    used.field(*axes[:4], shape=axes[4], exact=True)
    used.mesh_sparse(*axes, exact=True)
    used.set_option("exact", 1)
    used.set_option("exact", 0)
    got = answers(used)
    used.close()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g == w) if isinstance(g, str) else np.array_equal(g, w)
    assert not any("EXACT" in g for g in got if isinstance(g, str))


def test_the_walk_prunes(rm, pair):
    """The C5 scene (10 000 spheres) under the octree, 4 096 points on the first 4 096 spheres, no snap, no normal, no object:
    a lane evaluates n / 16 = 625 spheres on average at the most (leaves hold at most two spheres and best is near 0 at these
    points, so only boxes that almost contain the point survive), and the distances are the None context's."""
    ctx, ref = pair
    c, r = sphere_list(10000, 0x5EED5EED)
    ctx.set_option("exact", 0)
    ctx.scene_from_spheres(c, r, OCTREE)
    ref.scene_from_spheres(c, r, NONE)
    pts = (c[:4096].astype(np.float64) + r[:4096, None] * np.float64([0, 1, 0])).astype(np.float32)
    got = ctx.points(pts, normal=False, object=False, snap=0, exact=True)
    want = ref.points(pts, normal=False, object=False, snap=0)
    print("mean count %.2f, max %d (n = 10 000)" % (got.count.mean(), got.count.max()))
    assert got.count.mean() <= 625
    assert same(got.dist, want.dist)
    assert (want.count == 10000).all()


def test_refusals_with_a_device_and_no_scene(rm):
    N = rm._native
    ctx = rm.Context(0)
    ctx.set_option("exact", 1)
    with pytest.raises(rm.RmError) as e:
        ctx.points(np.zeros((4, 3), np.float32))
    assert e.value.code == N.RM_E_NO_SCENE
    with pytest.raises(rm.RmError) as e:
        ctx.field((0, 0, 0), (1, 0, 0), (0, 1, 0), shape=(4, 4))
    assert e.value.code == N.RM_E_NO_SCENE
    with pytest.raises(rm.RmError) as e:
        ctx.exact_tree()
    assert e.value.code == N.RM_E_NO_SCENE
    ctx.close()
