"""Sharp meshes on the GPU (rm_mesh_cells_device, rm_scene_sharpen_device, rm_scene_sharpen; Context.mesh_cells, sharpen and
sharp=True on the meshers).  The oracle is the numpy model of the rule (sharp_model.py) over the context's own distance
function -- Context.points with K = 0, which is rm_scene_distance, or the exact field with exact=True -- and there are no
tolerances: position, feature and count are compared byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_model as MM  # noqa: E402
import sharp_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, OCTREE, BVH = 0, 1, 2
BOX_AT, BOX_HALF, ROTATION = (0.03, -0.02, 0.01), (0.5, 0.35, 0.25), (0.4, 0.3, 0.2)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.view(np.uint8).tobytes() == b.view(np.uint8).tobytes()


def cube(n, half):
    """(origin, du, dv, dw, shape): n^3 points from -half to half."""
    step = 2.0 * half / (n - 1)
    return (-half, -half, -half), (step, 0, 0), (0, step, 0), (0, 0, step), (n, n, n)


# a sheared lattice whose (du, dv, dw) is left-handed (dw points down)
SHEARED = ((-1.1, -1.05, 1.0), (0.13, 0.01, 0.0), (0.02, 0.125, 0.0), (0.0, 0.015, -0.12), (18, 17, 18))


def distance(ctx, time=0.0, exact=False):
    """D of the model: the context's own getDistance at `time` -- Context.points with K = 0, no normal, no object."""
    def D(points):
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        if not len(points):
            return np.zeros(0, np.float64), np.zeros(0, np.uint64)
        r = ctx.points(points, normal=False, object=False, snap=0, time=time, exact=exact)
        return r.dist, r.count.astype(np.uint64)
    return D


def box_scene(rm, ctx, rotation, accel):
    ctx.scene_from_prims([(1, rm.make_transform(*BOX_AT, rotation=rotation), BOX_HALF)], accel)


def mixed_scene(rm, ctx, accel):
    from cpu_raymarcher_amd import synthetic as S
    ctx.scene_from_prims(S.mixed_prims_as_triples(S.synthetic_mixed_prims(12), rm.make_transform), accel)


def lattice_cells(ctx, lat, time=0.0, iso=0.0, exact=False):
    D = distance(ctx, time, exact)
    return SM.active_cells(SM.lattice_values(D, *lat[:4], *lat[4]), *lat[4], iso)


def check(ctx, lat, cells, time=0.0, iso=0.0, refine=2, rank_tol=0.1, reach=1.0, exact=False, what=None):
    """The host entry and the device entry against the model, byte for byte -> the model's result."""
    D = distance(ctx, time, exact)
    want = SM.sharpen(D, cells, *lat[:4], *lat[4], iso=iso, rank_tol=rank_tol, reach=reach, refine=refine)
    knobs = dict(iso=iso, time=time, refine=refine, rank_tol=rank_tol, reach=reach, exact=exact)
    host = ctx.sharpen(cells, *lat, **knobs)
    if len(cells):  # (no vertex, no launch)
        kernel = ctx.last_kernel()
        assert kernel.startswith("sharp_kernel<"), kernel
        assert ("EXACT" in kernel) == bool(exact), kernel
    dev = ctx.sharpen(cells, *lat, device=True, **knobs)
    for name, got in (("host", host), ("device", tuple(t.cpu().numpy() for t in dev))):
        differ = int((got[0] != want.position).any(axis=1).sum()) if len(cells) else 0
        assert same(got[0], want.position), (what, name, "position", differ, len(cells))
        assert same(got[1], want.feature), (what, name, "feature")
        assert np.array_equal(got[2].view(np.uint32).astype(np.uint64), want.count), (what, name, "count")
    return want


@pytest.fixture(scope="module")
def sctx(rm):
    ctx = rm.Context(0)
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ the rule, by scene

@pytest.mark.parametrize("rotation", [None, ROTATION], ids=["axis", "rotated"])
@pytest.mark.parametrize("accel", [NONE, BVH])
def test_a_box_equals_the_model(rm, sctx, rotation, accel):
    box_scene(rm, sctx, rotation, accel)
    lat = cube(17, 1.0)
    cells = lattice_cells(sctx, lat)
    assert len(cells) == (186 if rotation is None else 281)
    want = check(sctx, lat, cells, what=("box", rotation, accel))
    assert sctx.last_kernel() == "sharp_kernel<%d, 1>" % accel
    ranks = np.bincount(want.feature + 1, minlength=5)[1:]
    assert ranks[3] >= 5 and ranks[2] >= 50 and ranks[0] <= 1, ranks  # corners, edges; the fallback is rare


@pytest.mark.parametrize("exact", [False, True])
def test_mixed_primitives_under_the_octree_equal_the_model(rm, sctx, exact):
    mixed_scene(rm, sctx, OCTREE)
    lat = cube(26, 1.7)
    cells = lattice_cells(sctx, lat, exact=exact)
    assert len(cells) > 100
    want = check(sctx, lat, cells, exact=exact, what=("mixed", exact))
    assert (want.feature >= 0).all() and (want.feature >= 2).any()


def test_the_dense_grid_under_the_bvh_equals_the_model(rm, sctx):
    """Preset 3 at 17^3: the cell table and the step box of a sphere scene's BVH take their paths."""
    sctx.scene_from_preset(3, BVH)
    lat = cube(17, 1.6)
    cells = lattice_cells(sctx, lat)
    assert len(cells) >= 500
    check(sctx, lat, cells, what="dense grid")
    assert sctx.last_kernel() == "sharp_kernel<2, 0>"


def test_an_animated_operator_preset_equals_the_model_at_its_time(rm, sctx):
    sctx.scene_from_preset(12, OCTREE)
    lat = cube(17, 2.0)
    cells = lattice_cells(sctx, lat, time=0.7)
    assert len(cells) > 20
    want = check(sctx, lat, cells, time=0.7, what="animated")
    gen = int(sctx.last_kernel().split(",")[1].strip(" >"))
    assert gen in (2, 3), sctx.last_kernel()
    assert not same(sctx.sharpen(cells, *lat, time=0.0).position, want.position)  # the time matters


# ---------------------------------------------------------------------------------------------- the rule, by argument

@pytest.fixture(scope="module")
def rotated_box(rm, sctx):
    """The rotated box under the BVH on the 17^3 lattice: (lattice, cells); tests that use it load the scene themselves."""
    box_scene(rm, sctx, ROTATION, BVH)
    lat = cube(17, 1.0)
    return lat, lattice_cells(sctx, lat)


@pytest.mark.parametrize("refine", [0, 8])
def test_the_refinement_count_is_the_models(rm, sctx, rotated_box, refine):
    box_scene(rm, sctx, ROTATION, BVH)
    lat, cells = rotated_box
    check(sctx, lat, cells, refine=refine, what=("refine", refine))


@pytest.mark.parametrize("rank_tol,reach", [(0.0, 1.0), (1.0, 1.0), (0.1, 0.0), (0.3, 0.25)])
def test_the_rank_and_reach_knobs_are_the_models(rm, sctx, rotated_box, rank_tol, reach):
    box_scene(rm, sctx, ROTATION, BVH)
    lat, cells = rotated_box
    want = check(sctx, lat, cells, rank_tol=rank_tol, reach=reach, what=("knobs", rank_tol, reach))
    if rank_tol == 1.0 or reach == 0.0:
        assert (want.feature == 0).all()  # no eigenvalue exceeds the largest; no solution lies at the centre itself


def test_an_offset_surface_of_the_exact_field_equals_the_model(rm, sctx):
    mixed_scene(rm, sctx, BVH)
    lat = cube(26, 1.7)
    cells = lattice_cells(sctx, lat, iso=0.05, exact=True)
    assert len(cells) > 100 and not np.array_equal(cells, lattice_cells(sctx, lat, exact=True))
    check(sctx, lat, cells, iso=0.05, exact=True, what="offset")


def test_a_sheared_left_handed_lattice_equals_the_model(rm, sctx):
    box_scene(rm, sctx, ROTATION, BVH)
    u, v, w = (np.float64(x) for x in SHEARED[1:4])
    assert np.dot(u, np.cross(v, w)) < 0
    cells = lattice_cells(sctx, SHEARED)
    assert len(cells) > 150
    want = check(sctx, SHEARED, cells, what="sheared")
    assert (want.feature == 3).sum() >= 4


def test_keys_that_are_inactive_out_of_range_or_repeated(rm, sctx, rotated_box):
    box_scene(rm, sctx, ROTATION, BVH)
    lat, cells = rotated_box
    n = 17
    inactive = np.setdiff1d(np.arange(n ** 3), cells)
    inactive = inactive[(inactive % n < n - 1) & ((inactive // n) % n < n - 1) & (inactive // (n * n) < n - 1)]
    odd = np.array([-1, -2 ** 62, n ** 3, n ** 3 + 5, 2 ** 62, n - 1, n * n - 1, n ** 3 - 1], np.int64)  # the last three: no cell starts at a last point
    keys = np.concatenate([cells[:40], inactive[:5], odd, cells[:7], cells[30:50][::-1], inactive[-3:]]).astype(np.int64)
    want = check(sctx, lat, keys, what="keys")
    assert (want.feature[40:45] == -1).all() and (want.count[40:45] == 8).all()  # one primitive at each of the eight corners
    assert (want.feature[45:53] == -1).all() and not want.position[45:53].any() and not want.count[45:53].any()
    assert same(want.position[53:60], want.position[:7]) and (want.feature[:40] >= 0).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_vertex_counts_at_the_workgroup_edges(rm, sctx, rotated_box, n):
    box_scene(rm, sctx, ROTATION, BVH)
    lat, cells = rotated_box
    want = check(sctx, lat, cells[100:100 + n], what=("n", n))
    assert len(want.position) == n


def test_feature_and_count_are_optional(rm, sctx, rotated_box):
    import torch
    N = rm._native
    box_scene(rm, sctx, ROTATION, BVH)
    lat, cells = rotated_box
    full = sctx.sharpen(cells, *lat)
    l = rm.context.make_lattice(*lat)
    q = sctx._sharp_query(0.0, 2, 0.1, 1.0)
    n = len(cells)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    d_cells = torch.from_numpy(cells).cuda()
    for want_feature, want_count in ((False, False), (True, False), (False, True)):
        pos, feat, cnt = np.zeros((n, 3), np.float32), np.full(n, 77, np.int32), np.full(n, 77, np.uint32)
        N.check(sctx._h, N.lib().rm_scene_sharpen(sctx._h, C.byref(l), C.byref(q), n, vp(cells), vp(pos), vp(feat) if want_feature else None,
                                                  vp(cnt) if want_count else None))
        assert same(pos, full.position)
        assert same(feat, full.feature) if want_feature else (feat == 77).all()
        assert same(cnt, full.count) if want_count else (cnt == 77).all()
        dev = sctx._sharpen_device(l, d_cells, 0.0, 2, 0.1, 1.0, want_feature, want_count)
        assert same(dev[0].cpu().numpy(), full.position) and (dev[1] is None) == (not want_feature) and (dev[2] is None) == (not want_count)
        if want_feature:
            assert same(dev[1].cpu().numpy(), full.feature)
        if want_count:
            assert same(dev[2].cpu().numpy().view(np.uint32), full.count)


def test_a_host_batch_crosses_the_chunk_of_the_host_form(rm, sctx):
    """2^22 + 65 keys -- the active cells of a 17^3 lattice around the Sphere preset, repeated --, position and feature only: the
    host form takes 2^22 at a time, and the second trip ends in a partial workgroup of RM_SHARP_CELLS = 64 vertices."""
    import torch
    N = rm._native
    sctx.scene_from_preset(0, NONE)
    lat = cube(17, 2.0)
    active = lattice_cells(sctx, lat)
    assert len(active) > 100
    chunk, n = 1 << 22, (1 << 22) + 65
    keys = np.ascontiguousarray(np.resize(active, n), np.int64)
    l = rm.context.make_lattice(*lat)
    q = sctx._sharp_query(0.0, 2, 0.1, 1.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pos, feat = np.full((n, 3), np.nan, np.float32), np.full(n, -7, np.int32)
    N.check(sctx._h, N.lib().rm_scene_sharpen(sctx._h, C.byref(l), C.byref(q), n, vp(keys), vp(pos), vp(feat), None))
    assert sctx.last_kernel() == "sharp_kernel<0, 0>"
    d_pos, d_feat, d_cnt = sctx._sharpen_device(l, torch.from_numpy(keys).cuda(), 0.0, 2, 0.1, 1.0, True, False)
    assert d_cnt is None
    assert same(pos, d_pos.cpu().numpy()) and same(feat, d_feat.cpu().numpy())
    assert (feat >= 0).all() and np.isfinite(pos).all()
    for i in (0, chunk - 1, chunk, n - 1):
        one_pos, one_feat = np.zeros((1, 3), np.float32), np.zeros(1, np.int32)
        N.check(sctx._h, N.lib().rm_scene_sharpen(sctx._h, C.byref(l), C.byref(q), 1, vp(keys[i:i + 1]), vp(one_pos), vp(one_feat), None))
        assert same(one_pos, pos[i:i + 1]) and one_feat[0] == feat[i], i


# ------------------------------------------------------------------------------------------------- cells and meshers

def test_mesh_cells_are_the_active_cells_in_vertex_order(rm, sctx):
    N = rm._native
    mixed_scene(rm, sctx, BVH)
    lat = cube(26, 1.7)  # more than one block of the sparse mesher per axis, and a partial one
    shape = lat[4]
    vol, _ = sctx.field(*lat[:4], shape=shape, count=False)
    nets, _, holes = MM.mesh(vol.reshape(-1), *lat[:4], *shape)
    want = SM.active_cells(vol.reshape(-1), *shape)
    assert holes == 0 and len(want) == len(nets) > 200
    got = sctx.mesh_cells(vol, *lat)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert sctx.last_kernel() == "mesh_count_kernel<double>"
    assert np.array_equal(sctx.mesh_cells(vol.astype(np.float32), *lat), SM.active_cells(vol.astype(np.float32).reshape(-1), *shape))
    assert np.array_equal(sctx.mesh_cells(vol, *lat, iso=0.05), SM.active_cells(vol.reshape(-1), *shape, 0.05))
    # a capacity below the total: the first keys, the true total in info
    import torch
    l = rm.context.make_lattice(*lat)
    d_vol = torch.from_numpy(vol).cuda()
    few = torch.full((12,), -7, dtype=torch.int64, device="cuda")
    info = torch.zeros(4, dtype=torch.int64, device="cuda")
    N.check(sctx._h, N.lib().rm_mesh_cells_device(sctx._h, C.byref(l), d_vol.data_ptr(), N.RM_MESH_F64, 0.0, few.data_ptr(), 10, info.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(few.cpu().numpy()[:10], want[:10]) and (few.cpu().numpy()[10:] == -7).all()
    assert info.cpu().tolist()[0] == len(want) and info.cpu().tolist()[3] == 0
    # the sparse mesher's keys, sorted
    V = len(want)
    verts, quads, cells, minfo = np.zeros((V, 3), np.float32), np.zeros((4 * V, 4), np.uint32), np.zeros(V, np.int64), N.rm_mesh_info()
    N.check(sctx._h, N.lib().rm_scene_mesh_sparse(sctx._h, C.byref(l), 0.0, 1.0, verts.ctypes.data_as(C.c_void_p), V, quads.ctypes.data_as(C.c_void_p),
                                                  4 * V, cells.ctypes.data_as(C.c_void_p), None, C.byref(minfo), None))
    assert minfo.n_vertices == V and np.array_equal(np.sort(cells), want)
    # no cell: nothing
    assert len(sctx.mesh_cells(np.zeros((1, 5, 5)), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (5, 5, 1))) == 0


@pytest.mark.parametrize("lattice", ["cube", "sheared"])
def test_the_meshers_return_the_sharpened_vertices_and_the_same_faces(rm, sctx, lattice):
    box_scene(rm, sctx, ROTATION, BVH)
    lat = cube(17, 1.0) if lattice == "cube" else SHEARED
    plain_v, plain_q = sctx.mesh(*lat)
    sharp_v, sharp_q = sctx.mesh(*lat, sharp=True)
    assert same(sharp_q, plain_q) and not same(sharp_v, plain_v)
    cells = lattice_cells(sctx, lat)
    want = SM.sharpen(distance(sctx), cells, *lat[:4], *lat[4])
    assert same(sharp_v, want.position)
    sparse_v, sparse_q = sctx.mesh_sparse(*lat, sharp=True, order="dense")
    assert same(sparse_v, sharp_v) and same(sparse_q, sharp_q)
    tile_v, _ = sctx.mesh_sparse(*lat, sharp=True, order="tile")
    assert same(np.sort(tile_v.view("f4,f4,f4").reshape(-1)), np.sort(sharp_v.view("f4,f4,f4").reshape(-1)))
    # the knobs reach the pass; triangles and attributes come from the sharpened vertices
    loose_v, _ = sctx.mesh(*lat, sharp=True, refine=0, rank_tol=0.3, reach=0.5)
    assert same(loose_v, SM.sharpen(distance(sctx), cells, *lat[:4], *lat[4], refine=0, rank_tol=0.3, reach=0.5).position)
    v, tris, normals, objects = sctx.mesh(*lat, sharp=True, triangles=True, attributes=True)
    assert same(v, sharp_v) and len(tris) == 2 * len(sharp_q)
    at = sctx.points(sharp_v, normal=True, object=True)
    assert same(normals, at.normal) and same(objects, at.object)


def test_scene_to_mesh_and_mesh_box_take_the_option(rm):
    sc = rm.Scene("BVH", device=0)
    sc.loadPreset(3)
    plain_v, plain_q = sc.toMesh(cells=(12, 12, 12))
    sharp_v, sharp_q = sc.toMesh(cells=(12, 12, 12), sharp=True)
    assert same(sharp_q, plain_q) and sharp_v.shape == plain_v.shape and not same(sharp_v, plain_v)
    box_v, box_q = sc.ctx.mesh_box((12, 12, 12), sharp=True, sparse=True)
    assert same(box_v, sharp_v) and same(box_q, sharp_q)


def test_the_existing_entries_and_the_scene_time_are_left_alone(rm, sctx):
    """Context.mesh without `sharp` returns the same bytes before and after a sharpen call, and rm_scene_set_time's value is kept."""
    sctx.scene_from_preset(12, OCTREE)
    lat = cube(17, 2.0)
    sctx.scene_set_time(0.2)
    pts = np.random.default_rng(3).uniform(-2, 2, (64, 3)).astype(np.float32)
    d_before, _ = sctx.scene_distance(pts)
    before = sctx.mesh(*lat, time=0.7, attributes=True, snap=2)
    cells = lattice_cells(sctx, lat, time=0.7)
    r = sctx.sharpen(cells, *lat, time=0.7)
    assert (r.feature >= 0).all()
    after = sctx.mesh(*lat, time=0.7, attributes=True, snap=2)
    assert all(same(a, b) for a, b in zip(before, after))
    d_after, _ = sctx.scene_distance(pts)
    assert same(d_before, d_after) and not same(d_after, sctx.points(pts, normal=False, object=False, time=0.7).dist)
    assert sctx.get_option("exact") == 0
