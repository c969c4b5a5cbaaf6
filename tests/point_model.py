"""The rule of rm_scene_points (include/rm_raymarch.h) restated in numpy over a distance callable, for tests: the callable is
D(points float32 [m, 3]) -> (dist float64 [m], count [m]) -- Scene.getDistance and the primitives it evaluated -- from the
oracle (oracle_distance) for small sets or from Context.scene_distance (context_distance), which is pinned to the oracle
elsewhere, for larger ones.  numpy's binary64 +, -, *, /, sqrt and its float64 -> float32 conversion are IEEE operations with
round-to-nearest-even, the operations the rule names.  The object is not part of this model: tests take it from
single-object scenes (test_ray_pick.single_object_values / expected_ids)."""
import collections

import numpy as np

PointResult = collections.namedtuple("PointResult", "position dist normal steps count")


def oracle_distance(scene, time=0.0):
    """D over an oracle.OracleScene, one call per point."""
    def D(points):
        res = [scene.distance(p, time) for p in np.asarray(points, np.float32).reshape(-1, 3)]
        return np.array([r[0] for r in res], np.float64), np.array([r[1] for r in res], np.uint64)
    return D


def context_distance(ctx, time=0.0):
    """D over Context.scene_distance (rm_scene_distance) with the scene at `time`."""
    def D(points):
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        if not len(points):
            return np.zeros(0, np.float64), np.zeros(0, np.uint64)
        ctx.scene_set_time(time)
        d, c = ctx.scene_distance(points)
        return d, c.astype(np.uint64)
    return D


def gradient(D, p, d):
    """G(p, d): getNormal (raymarcher.ts:123-135) at the points p with its first evaluation taken as d -> (normal float32
    [m, 3], the primitives its three evaluations counted)."""
    n = np.zeros((len(p), 3), np.float32)
    count = np.zeros(len(p), np.uint64)
    for c in range(3):
        q = p.copy()
        q[:, c] = (p[:, c].astype(np.float64) - 0.01).astype(np.float32)
        dq, k = D(q)
        with np.errstate(all="ignore"):
            n[:, c] = (d - dq).astype(np.float32)
        count += k
    w = n.astype(np.float64)
    with np.errstate(all="ignore"):
        length = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
        positive = length > 0
        scale = np.where(positive, 1 / np.sqrt(np.where(positive, length, 1.0)), length)
        return (w * scale[:, None]).astype(np.float32), count


def points_model(D, points, snap=0, tol=1e-4, iso=0.0, normal=True):
    """The rule, every point at once: -> PointResult(position, dist, normal, steps, count), count exact (uint64 here)."""
    p = np.array(points, np.float32).reshape(-1, 3)
    n = len(p)
    d = np.zeros(n, np.float64)
    g = np.zeros((n, 3), np.float32)
    steps = np.zeros(n, np.int32)
    count = np.zeros(n, np.uint64)
    active = np.ones(n, bool)
    while active.any():
        idx = np.nonzero(active)[0]
        d[idx], k = D(p[idx])
        count[idx] += k
        with np.errstate(all="ignore"):
            r = d[idx] - iso
            step = (steps[idx] < snap) & (np.abs(r) > tol)  # (a NaN r: no step)
        visit = step | bool(normal)
        active[idx[~visit]] = False
        idx, r, step = idx[visit], r[visit], step[visit]
        if not len(idx):
            break
        g[idx], k = gradient(D, p[idx], d[idx])
        count[idx] += k
        move = step & ~(g[idx] == 0).all(axis=1)
        active[idx[~move]] = False
        idx, r = idx[move], r[move]
        with np.errstate(all="ignore"):
            p[idx] = (p[idx].astype(np.float64) + g[idx].astype(np.float64) * (-r)[:, None]).astype(np.float32)
        steps[idx] += 1
    return PointResult(p, d, g if normal else np.zeros((n, 3), np.float32), steps, count)
