"""The exterior candidate grid (option `ext`): all-primitive evaluations at points outside the BVH root box scan the
list of their grid cell instead of all N spheres.  It must never change a byte: distances and counts against the oracle's
getDistance, whole frames against the oracle and against `ext` 0, with the option combinations that take the other paths of
bvh_distance_wave (the sequential form, short hit lists, the one-ray-per-lane kernel).

rm_scene_distance runs the one-ray-per-lane kernels, which do not use the grid; the points of the distance test go through
rm_debug_wave_distance instead: the wave loop's own distance function, one point per lane, with the options of a render.

The orbit camera sits 3 from the origin and the grid reaches to 8.7 on every axis, which covers every point with t <= 10 of a
frame's rays: no render has an evaluation point beyond the grid (the reference's camera cannot be pulled back), so the lanes
beyond the grid are checked by the distance test only."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REACH = 8.7   # rm_scene_host.cpp build_exterior_grid: the grid covers the cube |x| <= 8.7
CELLS = 32


def dense_grid():
    off = (5 - 1) * 0.6 / 2   # sceneManager.ts "Dense Sphere Grid"
    c = np.array([(x * 0.6 - off, y * 0.6 - off, z * 0.6 - off) for x in range(5) for y in range(5) for z in range(5)], np.float64)
    return np.concatenate([c, np.full((125, 1), 0.15)], axis=1)


def mixed_list():
    rng = np.random.default_rng(2024)
    sp = np.concatenate([rng.uniform(-1.4, 1.4, size=(40, 3)), rng.uniform(0.05, 0.45, size=(40, 1))], axis=1)
    return sp.astype(np.float32).astype(np.float64)


def exterior_points(root):
    """~2e5 points outside the root box: uniform in the grid's region, on every cell boundary of one row of cells per axis with
    their binary32 neighbours, just outside the six root faces, and beyond the grid."""
    rng = np.random.default_rng(5)
    lo, hi = root[:3].astype(np.float64), root[3:].astype(np.float64)
    pts = [rng.uniform(-REACH, REACH, size=(120000, 3))]
    w = 2 * REACH / CELLS
    for axis in range(3):
        b = np.float32(-REACH + w * np.arange(CELLS + 1))
        b = np.concatenate([b, np.nextafter(b, np.float32(np.inf)), np.nextafter(b, np.float32(-np.inf))])
        for other in ((2.3, -3.1), (-7.9, 0.4), (1.45, 1.45)):
            p = np.empty((len(b), 3))
            p[:, axis] = b
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = other
            pts.append(p)
    for axis in range(3):
        for face, sign in ((lo[axis], -1), (hi[axis], 1)):
            p = rng.uniform(lo - 0.2, hi + 0.2, size=(4000, 3))
            f = np.float32(face)
            steps = rng.integers(1, 4, size=4000)
            v = np.full(4000, f, np.float32)
            for _ in range(3):
                v = np.where(steps > 0, np.nextafter(v, np.float32(sign * np.inf)), v)
                steps = steps - 1
            p[:, axis] = v
            p[2000:, axis] = face + sign * rng.uniform(1e-6, 0.05, size=2000)
            pts.append(p)
    far = rng.uniform(-14, 14, size=(30000, 3))
    pts.append(far[np.abs(far).max(axis=1) > REACH])
    edge = rng.uniform(-REACH, REACH, size=(6000, 3))   # on and next to the grid's outer faces
    k = rng.integers(0, 3, size=6000)
    v = np.where(rng.integers(0, 2, size=6000) > 0, np.float32(REACH), np.float32(-REACH)).astype(np.float32)
    v = np.where(rng.integers(0, 3, size=6000) == 0, v, np.nextafter(v, np.float32(0)))   # the face itself, or the last value inside
    edge[np.arange(6000), k] = v
    pts.append(edge)
    p = np.concatenate(pts).astype(np.float32)
    outside = ((p < lo.astype(np.float32)) | (p > hi.astype(np.float32))).any(axis=1)
    return np.ascontiguousarray(p[outside])


@pytest.mark.parametrize("name", ["dense", "mixed"])
def test_distances_outside_the_root_box(rm, oracle, name):
    """Every point through bvh_distance_wave (rm_debug_wave_distance) with `ext` 1, bit for bit the oracle's getDistance and its
    count; the same with the grid off, with the general (non-uniform) scan on the one-radius scene, without the leaf grid (then
    points inside the root box that lie in no leaf reach the exterior lookup too, and its unlisted cells), and without the
    interior candidate grid.  Last, 2e4 points inside the root box ride along, so that waves mix all the cases."""
    import ctypes as C
    sp = dense_grid() if name == "dense" else mixed_list()
    ref = oracle.OracleScene(accel="BVH", spheres=sp)
    root = ref.root_bounds()
    ext_pts = exterior_points(root)
    assert len(ext_pts) > 150000
    rng = np.random.default_rng(6)
    pts = np.ascontiguousarray(np.concatenate([ext_pts, rng.uniform(root[:3], root[3:], size=(20000, 3)).astype(np.float32)]))
    L = oracle.lib()
    want_d, want_c = np.empty(len(pts)), np.empty(len(pts), np.uint32)
    cnt = C.c_uint32(0)
    L.ro_set_time(0.0)
    for i in range(len(pts)):
        cnt.value = 0
        want_d[i] = L.ro_scene_distance(ref._h, pts[i].ctypes.data_as(C.c_void_p), C.byref(cnt))
        want_c[i] = cnt.value
    assert (want_c[:len(ext_pts)] == len(sp)).all()   # outside the root box: outside every leaf
    ctx = rm.Context(0)
    sc = rm.Scene("BVH", ctx=ctx)
    sc.loadSpheres(sp[:, :3], sp[:, 3])
    for opts in (dict(), dict(ext=0), dict(uniform=0), dict(grid=0), dict(nn=0), dict(coop=0), dict(grid=0, uniform=0, ext=1)):
        for k, v in {**dict(ext=1, uniform=1, grid=1, nn=2, coop=1, filter=1), **opts}.items():
            ctx.set_option(k, v)
        d, c = ctx.wave_distance(pts)
        bad = np.flatnonzero(d.view(np.uint64) != want_d.view(np.uint64))
        assert bad.size == 0, (opts, bad[:5], pts[bad[:5]], d[bad[:5]], want_d[bad[:5]])
        assert np.array_equal(c, want_c), opts
    ctx.close()


def load(rm, ctx, sp):
    sc = rm.Scene("BVH", ctx=ctx)
    sc.loadSpheres(sp[:, :3], sp[:, 3])
    return sc


def render(rm, sc, W, H, ang, repeat=1):
    """(depth, normal, sdf, iters, rgba, diagnostics) of one frame, all from the render kernel"""
    import torch
    dev = torch.device("cuda:0")
    ctx = sc.ctx
    sc.camera.setAngles(*ang)
    n = W * H
    for _ in range(repeat):
        d = torch.zeros(n, dtype=torch.uint8, device=dev)
        nr = torch.zeros(3 * n, dtype=torch.uint8, device=dev)
        s16 = torch.zeros(n, dtype=torch.int16, device=dev)
        i16 = torch.zeros(n, dtype=torch.int16, device=dev)
        rgba = torch.zeros(4 * n, dtype=torch.uint8, device=dev)
        acc = torch.full((4,), -1, dtype=torch.int64, device=dev)
        rm.SphereTracer().runRaymarcher(sc, d, nr, s16, i16, W, H, 0.0, shadedBuffer=rgba, shader="iteration-heatmap", diagnostics=acc)
        torch.cuda.synchronize()
    return (d.cpu().numpy(), nr.cpu().numpy(), s16.cpu().numpy().view(np.uint16), i16.cpu().numpy().view(np.uint16), rgba.cpu().numpy(),
            ctx.decode_acc(acc))


def oracle_frame(oracle, sp, W, H, ang):
    ref = oracle.OracleScene(accel="BVH", spheres=sp)
    ref.set_angles(*ang)
    d, n, s, i = ref.render(W, H)
    s64, i64 = s.astype(np.int64), i.astype(np.int64)
    diag = {"total_sdf": int(s64.sum()), "total_iters": int(i64.sum()), "max_sdf": int(s64.max()), "min_sdf": int(s64.min())}
    return d, n, s, i, oracle.shade("iteration-heatmap", d, n, s, i, W, H), diag


def same(a, b, what):
    for k in range(5):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert {k: a[5][k] for k in b[5]} == b[5], what


DEFAULTS = dict(kernel=2, ext=1, list_cap=32, filter=1, uniform=1, coop=1, specialise_v2_after=0)
# faces, an edge, a corner, and two oblique views: the overshooting rays leave the root box through each
CAMERAS = [(0.0, 0.0), (0.0, math.pi / 2), (0.0, math.pi / 4), (0.6155, math.pi / 4), (-0.9, 2.3), (1.5, 0.3)]


@pytest.mark.parametrize("name", ["dense", "mixed"])
def test_frames_are_the_same_bytes(rm, oracle, name):
    W, H = 160, 96
    sp = dense_grid() if name == "dense" else mixed_list()
    ctx = rm.Context(0)
    sc = load(rm, ctx, sp)
    for ang in CAMERAS:
        want = oracle_frame(oracle, sp, W, H, ang)
        if name == "dense":   # the case the grid is for occurs in the frame: pixels that hold an all-primitive evaluation
            assert int((want[2] >= 125).sum()) >= 300, ang
        for opts in (dict(), dict(ext=0), dict(kernel=1), dict(list_cap=2), dict(filter=0), dict(uniform=0), dict(coop=0), dict(ext=1, nn=0)):
            for k, v in {**DEFAULTS, "nn": 2, **opts}.items():
                ctx.set_option(k, v)
            same(render(rm, sc, W, H, ang), want, (name, ang, opts))
    ctx.close()


def test_the_kernel_compiled_for_the_configuration_uses_the_grid_too(rm, oracle):
    """After three launches of one configuration the wave loop is compiled with the configuration as literals (rm_v2_fields.h:
    the grid's origin, cell size, dimensions and switch among them): the frames in flight of the benchmark run in that kernel."""
    W, H = 160, 96
    sp = dense_grid()
    ctx = rm.Context(0)
    sc = load(rm, ctx, sp)
    want = oracle_frame(oracle, sp, W, H, (0.2, 0.5))
    for ext in (1, 0):
        ctx.set_option("ext", ext)
        got = render(rm, sc, W, H, (0.2, 0.5), repeat=5)
        assert "compiled in" in ctx.last_kernel(), ctx.last_kernel()
        same(got, want, ext)
    ctx.close()


def test_degenerate_scenes(rm, oracle):
    """A root box larger than the grid's region (a sphere of radius 30 around the camera: the builder refuses the grid) and 16
    identical spheres (every list holds all 16; every evaluation is a tie and takes the sequential form)."""
    W, H = 96, 64
    rng = np.random.default_rng(9)
    big = np.concatenate([rng.uniform(-1.5, 1.5, size=(24, 3)), rng.uniform(0.1, 0.4, size=(24, 1))], axis=1).astype(np.float32).astype(np.float64)
    big[0] = (0.0, 0.0, 0.0, 30.0)
    twins = np.tile(np.array([[0.25, -0.5, 0.125, 0.2]]), (16, 1))
    ctx = rm.Context(0)
    for sp in (big, twins):
        sc = load(rm, ctx, sp)
        for ang in ((0.2, 0.5), (-1.0, 3.0)):
            want = oracle_frame(oracle, sp, W, H, ang)
            for opts in (dict(), dict(ext=0), dict(kernel=1)):
                for k, v in {**DEFAULTS, **opts}.items():
                    ctx.set_option(k, v)
                same(render(rm, sc, W, H, ang), want, (ang, opts))
    ctx.close()
