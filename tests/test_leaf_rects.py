"""The leaf screen rectangles of the v2 bundle cull (option `rect_cull`; rm_kernels.h rm_leaf_rect), on the CPU.

A launch culls the BVH leaves of a 64-pixel batch by comparing the batch's pixel rectangle with a table of leaf rectangles that
its workgroups work out once for the launch's camera.  rm_debug_leaf_rects runs the kernel's own text on the host.  Checked
here, without a device:

 * conservativeness: for every sampled pixel and every leaf whose box the ray of that pixel hits -- BoundingBox.intersectRay
   (boundingBox.ts:69-105, restated below from the oracle's bbox_intersectRay) with tExit >= 0 and tEnter <= MAX_DIST, the
   condition of bvh.ts:145-165 -- the pixel lies inside the leaf's rectangle.  The rays are the ones runRaymarcher casts
   (rm_camera_rays, binary32 directions), from the camera's own position or from one placed inside the scene;
 * a leaf with a corner at or behind the camera plane has the whole frame;
 * a camera whose axes are not orthonormal has no table; neither has a scene beyond the leaf cap, nor option `rect_cull` 0;
 * tightness (a condition on the rule, not a measurement): on the Dense Sphere Grid under the golden camera the rectangles admit,
   per 8 x 8 batch, hardly more leaves than the plane rule they replace (restated below in binary32).
"""
import numpy as np
import pytest

F = np.float32
MAX_DIST = 10.0
WHOLE = (0, 65535, 0, 65535)
CAMERAS = {  # name: (pitch, yaw, where the camera is placed: None = where the angles put it)
    "golden": (0.0, 0.0, None),
    "pitch0.2-yaw0.3": (0.2, 0.3, None),
    "yaw1.2": (0.0, 1.2, None),
    "inside-root": (0.1, 0.4, "root"),
    "inside-leaf": (-0.3, 2.0, "leaf"),
}
FRAMES = {"64x64": (64, 64, 1), "250x130": (250, 130, 1), "3840x2160": (3840, 2160, 16)}  # width, height, every n-th pixel


def random_spheres(n, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.5, 1.5, (n, 3)).astype(F), rng.uniform(0.03, 0.1, n)


def load(ctx, scene):
    ctx.set_option("kernel", 2)  # (the nine-sphere grid would otherwise run in the one-ray-per-lane kernel)
    ctx.set_option("rect_cull", 1)
    if scene.startswith("preset"):
        ctx.scene_from_preset(int(scene[6:]), 2)
    else:
        ctx.scene_from_spheres(*random_spheres(int(scene[6:])), 2)


def boxes(ctx):
    """lo, hi float32 [nodes, 3] and the indices of the non-empty leaves, from the host builder's BVH table."""
    nodes = ctx.scene_table("bvh", from_device=False).reshape(-1, 32)
    lo, hi = nodes[:, 0:12].copy().view("<f4"), nodes[:, 16:28].copy().view("<f4")
    leaf = nodes[:, 28:32].copy().view("<i4").reshape(-1)
    return lo, hi, np.flatnonzero((leaf >= 0) & ((leaf & 0xFF) != 0))


def camera(rm, ctx, name):
    from cpu_raymarcher_amd.context import camera_from_angles
    pitch, yaw, where = CAMERAS[name]
    rot, origin = camera_from_angles(pitch, yaw)
    lo, hi, leaves = boxes(ctx)
    if where == "root":  # off-centre in the root box
        origin = (lo[0] + (hi[0] - lo[0]) * np.array([0.55, 0.45, 0.6], F)).astype(F)
    elif where == "leaf":  # the middle of a leaf
        k = leaves[len(leaves) // 2]
        origin = ((lo[k] + hi[k]) * F(0.5)).astype(F)
    return pitch, yaw, rot, origin


def intersect_ray(lo, hi, origin, d):
    """BoundingBox.intersectRay for rays d [n, 3] (binary32) from `origin` against boxes lo / hi [m, 3]: hit [n, m], tEnter, tExit."""
    o = origin.astype(np.float64)
    d = d.astype(np.float64)[:, None, :]
    par = np.abs(d) < 1e-10
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / d
        t0 = (lo.astype(np.float64)[None] - o) * inv
        t1 = (hi.astype(np.float64)[None] - o) * inv
    a, b = np.minimum(t0, t1), np.maximum(t0, t1)
    a = np.where(par, -np.inf, a)
    b = np.where(par, np.inf, b)
    outside = par & ((origin[None, None, :] < lo[None]) | (origin[None, None, :] > hi[None]))
    t_in, t_out = a.max(axis=2), b.min(axis=2)
    return ~outside.any(axis=2) & ~(t_in > t_out), t_in, t_out


@pytest.fixture(scope="module")
def ctx(rm):
    c = rm.Context(None)
    yield c
    c.close()


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("scene", ["preset3", "preset2", "random300"])
def test_every_pixel_whose_ray_hits_a_leaf_lies_in_its_rectangle(rm, ctx, scene, cam, frame):
    load(ctx, scene)
    W, H, step = FRAMES[frame]
    pitch, yaw, rot, origin = camera(rm, ctx, cam)
    lo, hi, leaves = boxes(ctx)
    assert ctx.rect_cull(rot, origin, W, H)["planned"]
    rects, nodes = ctx.leaf_rects(rot, origin, W, H)
    assert np.array_equal(nodes, leaves) and len(leaves) > (64 if scene == "random300" else 0)
    r = rects.astype(np.int64)
    xs = np.arange(0, W, step)
    hits = 0
    for y in range(0, H, step):
        _, d = rm.camera_rays(W, H, pitch, yaw, y, y + 1)
        hit, t_in, t_out = intersect_ray(lo[leaves], hi[leaves], origin, d[xs])
        hit &= (t_out >= 0.0) & (t_in <= MAX_DIST)
        inside = (xs[:, None] >= r[None, :, 0]) & (xs[:, None] <= r[None, :, 1]) & (y >= r[None, :, 2]) & (y <= r[None, :, 3])
        bad = hit & ~inside
        assert not bad.any(), "pixel (%d, %d) hits leaf %d outside its rectangle %s" % (
            xs[np.argwhere(bad)[0][0]], y, leaves[np.argwhere(bad)[0][1]], rects[np.argwhere(bad)[0][1]])
        hits += int(hit.sum())
    assert hits > 0  # the camera sees the scene


@pytest.mark.parametrize("scene", ["preset3", "random300"])
def test_a_leaf_with_a_corner_behind_the_camera_has_the_whole_frame(rm, ctx, scene):
    load(ctx, scene)
    lo, hi, leaves = boxes(ctx)
    seen = 0
    for cam in ("inside-root", "inside-leaf", "golden"):
        _, _, rot, origin = camera(rm, ctx, cam)
        rects, _ = ctx.leaf_rects(rot, origin, 250, 130)
        corners = np.stack([np.where([(c >> k) & 1 for k in range(3)], hi[leaves], lo[leaves]) for c in range(8)], axis=1)
        z = -((corners.astype(np.float64) - origin.astype(np.float64)) @ rot[6:9].astype(np.float64))  # [leaf, corner]
        behind = (z <= 0.0).any(axis=1)
        assert all(tuple(rects[k]) == WHOLE for k in np.flatnonzero(behind))
        assert (cam == "golden") == (not behind.any())  # the orbit camera has the scene in front of it
        in_front = (z > 1e-3).all(axis=1)
        assert not any(tuple(rects[k]) == WHOLE for k in np.flatnonzero(in_front))
        seen += int(behind.sum())
    assert seen > 0


def test_cameras_and_scenes_without_a_table(rm, ctx):
    from cpu_raymarcher_amd.context import camera_from_angles
    load(ctx, "preset3")
    rot, origin = camera_from_angles(0.2, 0.3)
    ok = ctx.rect_cull(rot, origin, 250, 130)
    assert ok["planned"] and ok["reason"] == 0 and ok["leaves"] == 64 and ok["max_leaves"] == 256
    for bad in (rot * F(1.001), rot + np.array([0, 0, 0, 1e-3, 0, 0, 0, 0, 0], F), np.where(np.arange(9) == 4, np.nan, rot).astype(F)):
        why = ctx.rect_cull(bad, origin, 250, 130)  # scaled, sheared, not finite
        assert not why["planned"] and why["reason"] == 3
        assert len(ctx.leaf_rects(bad, origin, 250, 130)[0]) == 0
    assert ctx.rect_cull(rot, np.array([np.inf, 0, 0], F), 250, 130)["reason"] == 3
    assert ctx.rect_cull(rot, origin, 65537, 130)["reason"] == 3 and ctx.rect_cull(rot, origin, 65536, 65536)["planned"]
    ctx.set_option("rect_cull", 0)
    assert ctx.rect_cull(rot, origin, 250, 130)["reason"] == 1 and len(ctx.leaf_rects(rot, origin, 250, 130)[0]) == 0
    ctx.set_option("rect_cull", 1)
    ctx.set_option("cull", 0)
    assert ctx.rect_cull(rot, origin, 250, 130)["reason"] == 1
    ctx.set_option("cull", 1)
    ctx.scene_from_preset(3, 1)  # an octree has no leaf table
    assert ctx.rect_cull(rot, origin, 250, 130)["reason"] == 1
    load(ctx, "random2000")  # beyond the cap
    why = ctx.rect_cull(rot, origin, 250, 130)
    assert ctx.scene_info()["bvh_leaves"] > why["max_leaves"] and not why["planned"] and why["reason"] == 2
    assert len(ctx.leaf_rects(rot, origin, 250, 130)[0]) == 0
    load(ctx, "random300")
    assert ctx.rect_cull(rot, origin, 250, 130)["planned"] and 64 < ctx.rect_cull(rot, origin, 250, 130)["leaves"] <= 256


def plane_rule(lo, hi, origin, rot, W, H, x0, x1, y0, y1):
    """The plane cull of rm_render_v2.hip (make_bundle, bundle_misses_box) in binary32 for batches [x0, x1] x [y0, y1] (arrays [b])
    against boxes [m]: admitted [b, m]."""
    mu, mv = max(F(1.0) / F(W), F(1e-4)), max(F(1.0) / F(H), F(1e-4))
    u0 = (x0.astype(F) / F(W) - F(0.5)) * F(2.0) - mu
    u1 = (x1.astype(F) / F(W) - F(0.5)) * F(2.0) + mu
    v0 = (y0.astype(F) / F(H) - F(0.5)) * F(2.0) - mv
    v1 = (y1.astype(F) / F(H) - F(0.5)) * F(2.0) + mv
    ql, qh = (lo - origin).astype(F), (hi - origin).astype(F)
    miss = np.zeros((len(x0), len(lo)), bool)
    for p, (t, col) in enumerate(((u0, 0), (u1, 0), (v0, 3), (v1, 3))):
        mx = np.zeros(miss.shape, F)
        mn = np.zeros(miss.shape, F)
        mag = np.zeros(miss.shape, F)
        for k in range(3):
            n = (rot[col + k] + t * rot[6 + k]).astype(F)[:, None]
            a, c = ql[None, :, k] * n, qh[None, :, k] * n
            mx = mx + np.maximum(a, c)
            mn = mn + np.minimum(a, c)
            mag = mag + np.maximum(np.abs(a), np.abs(c))
        tol = F(1e-6) * mag
        miss |= (mn > tol) if p & 1 else (mx < -tol)
    return ~miss


def test_rectangles_admit_hardly_more_than_the_plane_rule(rm, ctx):
    """Dense Sphere Grid, golden camera, the 4K frame of the benchmark, every 8 x 8 batch.  In exact arithmetic the two rules are
    the same rule.  The rectangles' pixel bounds are rounded outwards, by less than a pixel and 1e-6 of the frame a side: a
    leaf's rectangle reaches at most one more column of batches on either side, and one more row above and below, than the
    planes admit.  A leaf the planes give a columns and b rows of batches therefore gets at most (a + 2)(b + 2) pairs, cut off
    at the frame: the bound, summed over the leaves once the plane rule's own count is known (a factor of 1.06 here;
    expected is a small part of that, an edge crosses a batch boundary one time in eight)."""
    load(ctx, "preset3")
    W, H = 3840, 2160
    _, _, rot, origin = camera(rm, ctx, "golden")
    lo, hi, leaves = boxes(ctx)
    rects, _ = ctx.leaf_rects(rot, origin, W, H)
    r = rects.astype(np.int64)
    bx, by = np.meshgrid(np.arange(0, W, 8), np.arange(0, H, 8))
    x0, y0 = bx.ravel(), by.ravel()
    x1, y1 = x0 + 7, y0 + 7
    by_rect = (x0[:, None] <= r[None, :, 1]) & (x1[:, None] >= r[None, :, 0]) & (y0[:, None] <= r[None, :, 3]) & (y1[:, None] >= r[None, :, 2])
    by_plane = np.concatenate([plane_rule(lo[leaves], hi[leaves], origin, rot, W, H, x0[k:k + 8192], x1[k:k + 8192], y0[k:k + 8192], y1[k:k + 8192])
                               for k in range(0, len(x0), 8192)])
    grid = by_plane.reshape(by.shape[0], by.shape[1], len(leaves))
    a, b = grid.any(axis=0).sum(axis=0), grid.any(axis=1).sum(axis=0)  # batch columns / rows the planes admit, per leaf
    assert (a > 0).all() and (grid.sum(axis=(0, 1)) == a * b).all()  # (every leaf is on screen, as a block of batches)
    bound = int((np.minimum(a + 2, by.shape[1]) * np.minimum(b + 2, by.shape[0])).sum())
    n_rect, n_plane = int(by_rect.sum()), int(by_plane.sum())
    print("admitted (batch, leaf) pairs: rectangles %d, planes %d, ratio %.4f, bound %.4f; per batch %.3f against %.3f; batches without a "
          "candidate %.1f %%" % (n_rect, n_plane, n_rect / n_plane, bound / n_plane, n_rect / len(x0), n_plane / len(x0),
                                 100.0 * (~by_rect.any(axis=1)).mean()))
    assert n_rect <= bound
    assert not (by_plane & ~by_rect).any()  # and they admit no less: the same margins, the bounds rounded outwards
    assert by_rect.any(axis=1).mean() < 0.85  # a fifth of this frame's batches see no leaf at all: the rule finds them
