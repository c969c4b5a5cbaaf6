"""A numpy restatement of the reuse rule of rm_scene_tiles_update_device (include/rm_raymarch.h, "re-meshing an edited scene"),
operation for operation and taking nothing from the library: which kept blocks of the new scene copy their previous tile and
which are evaluated again.  Inputs: the previous slot map and tiles, the new list, the balls, the lattice.  Output: the flags
(1 copied, 0 evaluated), what the entry writes to d_reused."""
import numpy as np

import mesh_sparse_model as S


def half_widths(origin, du, dv, dw, nu, nv, nw):
    """float64 [3]: what a tile point is away from the tile's centre point at most, per axis -- four steps and the slack."""
    _, u, v, w = S._vectors(origin, du, dv, dw)
    slack = S.bound(origin, du, dv, dw, nu, nv, nw, 0.0)
    return np.array([np.float64(4.0) * ((abs(u[c]) + abs(v[c])) + abs(w[c])) + slack for c in range(3)], np.float64)


def tile_centres(origin, du, dv, dw, nu, nv, nw, lst):
    """float32 [n_kept, 3]: the lattice's point rule at index 8 b + 4 per axis, NOT clamped to the lattice."""
    nbu, nbv, _ = S.lattice_blocks(nu, nv, nw)
    b = np.asarray(lst, np.int64)
    bx, by, bz = b % nbu, (b // nbu) % nbv, b // (nbu * nbv)
    return S._points(origin, du, dv, dw, S.B * bx + 4, S.B * by + 4, S.B * bz + 4).reshape(-1, 3)


def as_balls(balls):
    """(float64 [n, 3] widened binary32 centres, float64 [n] radii) from a record array (center, radius) or pairs."""
    if isinstance(balls, np.ndarray) and balls.dtype.names:
        return balls["center"].astype(np.float32).astype(np.float64).reshape(-1, 3), balls["radius"].astype(np.float64).reshape(-1)
    c = np.array([np.asarray(b[0], np.float32) for b in balls], np.float32).reshape(-1, 3).astype(np.float64)
    return c, np.array([float(b[1]) for b in balls], np.float64)


def reused(prev_slot, prev_tiles, lst, balls, origin, du, dv, dw, nu, nv, nw):
    """int32 [n_kept]: 1 where the block's previous tile is copied, 0 where the block is evaluated."""
    prev_slot = np.asarray(prev_slot, np.int64)
    prev_tiles = np.asarray(prev_tiles, np.float64).reshape(-1, S.TILE)
    lst = np.asarray(lst, np.int64)
    n_blocks, n_prev = len(prev_slot), len(prev_tiles)
    out = np.zeros(len(lst), np.int32)
    if not len(lst):
        return out
    cb, rho = as_balls(balls)
    centre = tile_centres(origin, du, dv, dw, nu, nv, nw, lst).astype(np.float64)
    half = half_widths(origin, du, dv, dw, nu, nv, nw)
    inside = S.tile_indices(nu, nv, nw, lst) >= 0
    k1, k2 = np.float64(1.0) - np.float64(2.0 ** -20), np.float64(2.0 ** -20)
    with np.errstate(all="ignore"):
        for r, b in enumerate(lst):
            p = prev_slot[b] if 0 <= b < n_blocks else -1       # 1
            if p < 0 or p >= n_prev:
                continue
            c = centre[r]
            if not np.isfinite(c).all():                         # 2
                continue
            v = prev_tiles[p][inside[r]]                         # 3
            if np.isnan(v).any():
                continue
            M = v.max() if v.size else -np.inf
            lo, hi = c - half, c + half                          # 4
            e = np.maximum(np.maximum(lo - cb, cb - hi), 0.0)
            gap = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
            reach = ~(gap * k1 - k2 - rho > M)
            if reach.any():
                continue
            out[r] = 1                                           # 5
    return out


def edit_balls(centers, radii, edits):
    """What rm_scene_edit_balls writes for `edits` (as Context.edit_spheres takes them) on the list (centers, radii): for SET
    the sphere before and after, for INSERT the new one, for REMOVE the old one, in edit order -> [(centre float32[3], radius)]."""
    c = [np.asarray(row, np.float32) for row in np.asarray(centers, np.float32).reshape(-1, 3)]
    r = [float(v) for v in np.asarray(radii, np.float64).reshape(-1)]
    out = []
    for e in edits:
        op, i = e[0], int(e[1])
        if op != "insert":
            out.append((c[i], r[i]))
        if op == "remove":
            del c[i], r[i]
            continue
        centre, radius = np.asarray(e[2], np.float32), float(e[3])
        if op == "insert":
            c.insert(i, centre)
            r.insert(i, radius)
        else:
            c[i], r[i] = centre, radius
        out.append((centre, radius))
    return out
