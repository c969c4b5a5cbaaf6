"""rm_scene_edit_spheres on the device: the four tables the device builder (csrc/rm_scene_build.hip) supplies -- nn_cells /
nn_list, ext_cells / ext_list, oct_sub_hdr / oct_sub_list and the empty octree nodes' min_distance inside `oct` -- are the host
builder's, byte for byte, at the smallest inputs at which each kernel can go wrong; renders, distances and picks of an edited
scene are those of a freshly uploaded one; the device's binary64 Math.hypot is the host's.  The oracle of every case is
rm_scene_from_spheres(final list): the host builder, which no upload entry lets the device builder near."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_edit_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

MOVE = (0.07, -0.03, 0.11)


def moved(start, i, by=MOVE):
    c = start[0][i].astype(np.float64) + np.array(by)
    return [("set", i, tuple(c), float(start[1][i]))]


def grown(full):
    """(start, edits): `full` without its last sphere, and the INSERT that appends it"""
    return (full[0][:-1], full[1][:-1]), [("insert", len(full[1]) - 1, tuple(full[0][-1]), float(full[1][-1]))]


def crowded(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 0.25, (n, 3)).astype(np.float32), np.full(n, 0.01)


def synthetic(n):
    from cpu_raymarcher_amd.synthetic import synthetic_spheres
    s = synthetic_spheres(n)
    return np.ascontiguousarray(s[:, :3], np.float32), np.ascontiguousarray(s[:, 3], np.float64)


def cases():
    out = {}
    grid = M.dense_grid()
    out["bvh_125_one_moved"] = (M.BVH, grid, moved(grid, 62))  # two lane chunks with a ragged tail, the 48^3 grid, the exterior grid
    s16 = M.random_spheres(16, seed=3)
    out["bvh_15_to_16"] = (M.BVH,) + grown(s16)  # the exterior grid appears ...
    out["bvh_16_to_15"] = (M.BVH, s16, [("remove", 7)])      # ... and disappears
    out["bvh_64"] = (M.BVH,) + grown(M.random_spheres(64, seed=4))  # the lane-chunk boundary
    out["bvh_65"] = (M.BVH,) + grown(M.random_spheres(65, seed=5))
    one = (np.array([[0.3, -0.2, 0.1]], np.float32), np.array([0.5]))
    out["bvh_one_sphere_of_radius_0"] = (M.BVH, one, [("set", 0, (0.3, -0.2, 0.1), 0.0)])  # root box of zero extent: one cell per axis, *_inv = 0
    two = M.random_spheres(2, seed=6)
    out["bvh_1"] = (M.BVH, two, [("remove", 0)])
    same = (np.tile(np.array([[0.2, 0.1, -0.3]], np.float32), (300, 1)), np.full(300, 0.25))
    out["bvh_300_equal"] = (M.BVH,) + grown(same)  # every cell has >= 255 candidates: every header 255, both lists empty
    out["bvh_2048"] = (M.BVH,) + grown(synthetic(2048))  # the limit of the candidate grids; the grid side shrinks to 24
    out["bvh_2049"] = (M.BVH,) + grown(synthetic(2049))  # beyond it: the tables are empty
    s40 = M.random_spheres(40, seed=7)
    empty = (np.zeros((0, 3), np.float32), np.zeros(0))
    out["bvh_from_empty"] = (M.BVH, empty, [("insert", k, tuple(s40[0][k]), float(s40[1][k])) for k in range(40)])
    out["oct_125_one_moved"] = (M.OCTREE, grid, moved(grid, 62))  # empty nodes: nearest_prim_box
    far = (np.array([[-6, -6, -6], [6, -6, 5], [-5, 6, 6], [6, 6, -6], [0.5, 0.5, 0.5]], np.float32), np.array([0.3, 0.4, 0.2, 0.5, 0.1]))
    out["oct_5_far_apart"] = (M.OCTREE, far, moved(far, 4))  # the first split; most children are empty leaves
    c40, c300 = crowded(40, seed=8), crowded(300, seed=9)
    out["oct_40_crowded"] = (M.OCTREE, c40, moved(c40, 13, (0.004, -0.003, 0.002)))  # one depth-6 leaf above 8 spheres: sub-cell lists
    out["oct_300_crowded"] = (M.OCTREE, c300, moved(c300, 13, (0.004, -0.003, 0.002)))  # a leaf above 255 is skipped
    s2000 = synthetic(2000)
    out["oct_2000"] = (M.OCTREE, s2000, moved(s2000, 1234))  # many crowded leaves, about a thousand empty nodes
    return out


CASES = cases()


@pytest.fixture(scope="module")
def ctxs(rm):
    """The context that is edited and the one that uploads the final list (the oracle), on the GPU."""
    edited, fresh = rm.Context(0), rm.Context(0)
    yield edited, fresh
    edited.close()
    fresh.close()


def build_both(ctxs, name, device_build):
    edited, fresh = ctxs
    accel, start, edits = CASES[name]
    final = M.apply_edits(start[0], start[1], edits)
    fresh.scene_from_spheres(final[0], final[1], accel)
    edited.set_option("device_build", device_build)
    edited.scene_from_spheres(start[0], start[1], accel)
    edited.edit_spheres(edits)
    return accel, final


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_built_tables_are_the_host_builders(ctxs, name):
    edited, fresh = ctxs
    for device_build in (1, 0):
        build_both(ctxs, name, device_build)
        want = M.snapshot(fresh, True)
        M.assert_same(M.snapshot(edited, True), want, "%s, device_build = %d" % (name, device_build))
        M.assert_same(M.snapshot(edited, False), M.snapshot(fresh, False), "%s, host copy, device_build = %d" % (name, device_build))
    edited.set_option("device_build", 1)


def test_the_cases_reach_what_they_are_for(ctxs):
    """The inputs above do hit the paths they name (read from the oracle context: host-built tables)."""
    fresh = ctxs[1]

    def tables(name):
        build_both(ctxs, name, 1)
        return {t: fresh.scene_table(t) for t in ("nn_cells", "nn_list", "ext_cells", "ext_list", "oct_sub_hdr", "oct_sub_list")}, fresh.scene_info()

    t, _ = tables("bvh_125_one_moved")
    assert t["nn_cells"].size == 48 ** 3 and t["ext_cells"].size == 32 ** 3 and t["nn_list"].size and t["ext_list"].size
    assert tables("bvh_15_to_16")[0]["ext_cells"].size > 0 and tables("bvh_16_to_15")[0]["ext_cells"].size == 0
    t, _ = tables("bvh_one_sphere_of_radius_0")
    assert t["nn_cells"].size == 1
    t, _ = tables("bvh_300_equal")
    assert (t["nn_cells"] == 255).all() and t["nn_list"].size == 0 and t["ext_list"].size == 0
    # (exterior cells further than 10 from the spheres list nothing -- header 0 --, every other one is crowded)
    assert np.isin(t["ext_cells"], (0, 255)).all() and (t["ext_cells"] == 255).any()
    assert tables("bvh_2048")[0]["nn_cells"].size == 24 ** 3 and tables("bvh_2049")[0]["nn_cells"].size == 0
    t, info = tables("oct_125_one_moved")
    assert info["oct_empty_leaves"] > 0
    t, info = tables("oct_40_crowded")
    assert t["oct_sub_hdr"].size == 12 ** 3 and info["oct_max_leaf_prims"] == 40
    t, info = tables("oct_300_crowded")
    assert info["oct_max_leaf_prims"] > 255
    t, info = tables("oct_2000")
    assert t["oct_sub_hdr"].size >= 10 * 12 ** 3 and info["oct_empty_leaves"] >= 500


def observe(ctx, rm, accel):
    """A 64 x 64 render (all four buffers), distances over a 16^3 lattice through the scene and picks of the camera rays."""
    N = rm.context.N
    job = N.rm_job()
    job.width = job.height = job.y_end = 64
    job.camera_pitch, job.camera_yaw = 0.2, 0.5
    job.algorithm = N.lib().rm_algorithm_from_string(b"sphere-tracer")
    job.scene_preset_index = N.RM_SCENE_UPLOADED
    job.acceleration_structure = accel
    job.overshoot_factor = job.step_size = float("nan")
    bufs = [np.zeros(64 * 64, np.uint8), np.zeros(64 * 64 * 3, np.uint8), np.zeros(64 * 64, np.uint16), np.zeros(64 * 64, np.uint16)]
    ctx.render_tile(job, *bufs)
    g = np.linspace(-1.6, 1.6, 16)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    dist, cnt = ctx.scene_distance(pts)
    o, d, _ = ctx._frame_rays(64, 64, 0.2, 0.5, 0, None, False)
    picks = ctx.pick(o, d)
    return [b.tobytes() for b in bufs] + [dist.tobytes(), cnt.tobytes()] + [np.asarray(p).tobytes() for p in picks], picks[4]


@pytest.mark.parametrize("name", ["bvh_125_one_moved", "oct_125_one_moved", "oct_40_crowded"])
def test_an_edited_scene_behaves_like_an_uploaded_one(rm, ctxs, name):
    edited, fresh = ctxs
    accel, final = build_both(ctxs, name, 1)
    got, objects = observe(edited, rm, accel)
    want, _ = observe(fresh, rm, accel)
    assert got == want
    assert objects.max() < len(final[1]) and (objects.max() >= 0 or name == "oct_40_crowded")  # (spheres of radius 0.01: below a pixel)
    if name == "bvh_125_one_moved":  # object order, not device slots: down the column x = y = -1.2 the first hit is object 4 (z = 1.2)
        down = edited.pick(np.array([[-1.2, -1.2, 5.0]], np.float32), np.array([[0, 0, -1]], np.float32))
        assert int(down[4][0]) == 4
    # a job that names another acceleration structure rebuilds the edited list, not the old one
    other = M.OCTREE if accel == M.BVH else M.BVH
    assert observe(edited, rm, other)[0] == observe(fresh, rm, other)[0]
    assert edited.scene_info()["n_prims"] == len(final[1])


def test_device_hypot64_is_the_hosts(ctxs):
    """10 000 triples of differences of random binary32 values, with zeros and with one component dominating by 2^60."""
    rng = np.random.default_rng(12)
    a = (rng.standard_normal((10000, 3)) * np.exp2(rng.integers(-20, 20, (10000, 3)))).astype(np.float32)
    b = (rng.standard_normal((10000, 3)) * np.exp2(rng.integers(-20, 20, (10000, 3)))).astype(np.float32)
    x = a.astype(np.float64) - b.astype(np.float64)
    x[rng.random((10000, 3)) < 0.15] = 0.0
    x[:50] = 0.0  # all three zero
    big = rng.integers(0, 3, 2000)
    x[100:2100][np.arange(2000), big] *= 2.0 ** 60
    x[2100:2200] *= 2.0 ** -40
    edited = ctxs[0]
    dev, host = edited.selftest_hypot64(x, True), edited.selftest_hypot64(x, False)
    assert np.array_equal(dev.view(np.uint64), host.view(np.uint64))
    assert (host[:50] == 0).all() and np.isfinite(host).all() and (host[100:2100] > 0).any()
