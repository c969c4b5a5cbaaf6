"""What tests/test_scene_edit.py and tests/test_scene_edit_gpu.py share: the rule of rm_scene_edit_spheres on a Python list,
a snapshot of every scene table, and the sphere lists the cases start from."""
import numpy as np

NONE, OCTREE, BVH = 0, 1, 2


def apply_edits(centers, radii, edits):
    """The edited list: edits as Context.edit_spheres takes them, applied in order; indices at the moment of each edit."""
    c = [tuple(np.float32(v) for v in row) for row in np.asarray(centers, np.float32).reshape(-1, 3)]
    r = [float(v) for v in np.asarray(radii, np.float64).reshape(-1)]
    for e in edits:
        op, i = e[0], int(e[1])
        if op == "remove":
            assert 0 <= i < len(r)
            del c[i], r[i]
            continue
        centre, radius = tuple(np.float32(v) for v in e[2]), float(e[3])
        if op == "insert":
            assert 0 <= i <= len(r)
            c.insert(i, centre)
            r.insert(i, radius)
        else:
            assert op == "set" and 0 <= i < len(r)
            c[i], r[i] = centre, radius
    return np.array(c, np.float32).reshape(-1, 3), np.array(r, np.float64)


def table_names():
    from cpu_raymarcher_amd import _native  # (loads the library: not at import time, the `rm` fixture builds it first)
    return sorted(_native.SCENE_TABLES)


def snapshot(ctx, from_device):
    """Every scene table's bytes and rm_scene_get_info: what two contexts with the same scene agree on."""
    snap = {name: ctx.scene_table(name, from_device=from_device).tobytes() for name in table_names()}
    snap["info"] = ctx.scene_info()
    return snap


def assert_same(got, want, what=""):
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    for name in table_names():
        if got[name] != want[name]:
            a, b = np.frombuffer(got[name], np.uint8), np.frombuffer(want[name], np.uint8)
            where = int(np.argmax(a[:min(a.size, b.size)] != b[:min(a.size, b.size)])) if min(a.size, b.size) else 0
            raise AssertionError("%s: table %s differs (%d against %d bytes, first difference at byte %d)"
                                 % (what, name, a.size, b.size, where))


def dense_grid():
    """Preset 3 (sceneManager.ts "Dense Sphere Grid"): 5^3 spheres of radius 0.15, spacing 0.6."""
    c = [(x * 0.6 - 1.2, y * 0.6 - 1.2, z * 0.6 - 1.2) for x in range(5) for y in range(5) for z in range(5)]
    return np.array(c, np.float64).astype(np.float32), np.full(125, 0.15)


def random_spheres(n, seed, lo=-1.5, hi=1.5, rmin=0.05, rmax=0.3):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32), rng.uniform(rmin, rmax, n)
