"""A numpy restatement of the sparse-mesh rule of include/rm_raymarch.h ("sparse meshes"), taking nothing from the library:
the blocks of a lattice and their centres, the bound and the keep rule, the slots and the list, the tiles, and surface nets
over the kept blocks -- the dense rule of tests/mesh_model.py with "a cell of a block that was not kept is not active", the
vertices in (slot, local cell) order, the quads in (slot, 3 local + A) order, and the dense mesher's sort keys beside them.
The distances at the centres are an input: the rule says which value they are (the exact field), not how to compute it."""
import numpy as np

from mesh_model import CYCLIC, EDGES

B = 8
TILE = 729
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]


def axis_blocks(n):
    return (n - 1 + B - 1) // B if n >= 2 else 0


def lattice_blocks(nu, nv, nw):
    return axis_blocks(nu), axis_blocks(nv), axis_blocks(nw)


def _vectors(origin, du, dv, dw):
    return tuple(np.asarray(x, np.float32).astype(np.float64) for x in (origin, du, dv, dw))


def _points(origin, du, dv, dw, i, j, k):
    """The lattice's point rule at integer index arrays: binary64, left to right, one rounding to binary32 -> [..., 3]."""
    o, u, v, w = _vectors(origin, du, dv, dw)
    fi, fj, fk = (np.asarray(x).astype(np.float64) for x in (i, j, k))
    out = np.empty(fi.shape + (3,), np.float32)
    for c in range(3):
        s = o[c] + fi * u[c]
        s = s + fj * v[c]
        s = s + fk * w[c]
        out[..., c] = s.astype(np.float32)
    return out


def centres(origin, du, dv, dw, nu, nv, nw):
    """float32 [n_blocks, 3]: the centre of every block in block order."""
    nbu, nbv, nbw = lattice_blocks(nu, nv, nw)
    bz, by, bx = np.meshgrid(np.arange(nbw), np.arange(nbv), np.arange(nbu), indexing="ij")
    i, j, k = np.minimum(B * bx + 4, nu - 1), np.minimum(B * by + 4, nv - 1), np.minimum(B * bz + 4, nw - 1)
    return _points(origin, du, dv, dw, i, j, k).reshape(-1, 3)


def bound(origin, du, dv, dw, nu, nv, nw, lipschitz):
    o, u, v, w = _vectors(origin, du, dv, dw)

    def norm(x):
        return np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])

    R = np.float64(4.0) * ((norm(u) + norm(v)) + norm(w))
    last = [max(n - 1, 0) for n in (nu, nv, nw)]
    corners = [_points(origin, du, dv, dw, np.array(a * last[0]), np.array(b * last[1]), np.array(c * last[2]))
               for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    M = np.float64(max(float(np.abs(p.astype(np.float64)).max()) for p in corners))
    slack = M * np.float64(2.0 ** -20)
    return np.float64(lipschitz) * R + slack


def blocks(dist, iso, bnd):
    """(slot int32 [n_blocks], list int32 [n_kept]) from the exact distances at the centres."""
    d = np.asarray(dist, np.float64)
    with np.errstate(invalid="ignore"):
        keep = ~(np.abs(d - np.float64(iso)) > bnd)  # NaN keeps
    lst = np.nonzero(keep)[0].astype(np.int32)
    slot = np.full(len(d), -1, np.int32)
    slot[lst] = np.arange(len(lst), dtype=np.int32)
    return slot, lst


def tile_indices(nu, nv, nw, lst):
    """int64 [n_kept, 729]: the linear index of every tile point, -1 beyond the lattice."""
    nbu, nbv, _ = lattice_blocks(nu, nv, nw)
    b = np.asarray(lst, np.int64)
    if not len(b):
        return np.zeros((0, TILE), np.int64)
    bx, by, bz = b % nbu, (b // nbu) % nbv, b // (nbu * nbv)
    t = np.arange(TILE)
    ta, tb, tg = t % 9, (t // 9) % 9, t // 81
    i, j, k = B * bx[:, None] + ta, B * by[:, None] + tb, B * bz[:, None] + tg
    return np.where((i < nu) & (j < nv) & (k < nw), (k * nv + j) * nu + i, -1)


def tiles(values, nu, nv, nw, lst):
    idx = tile_indices(nu, nv, nw, lst)
    v = np.asarray(values, np.float64).reshape(-1)
    out = np.where(idx >= 0, v[np.maximum(idx, 0)], QNAN) if v.size else np.full(idx.shape, QNAN)
    return out.astype(np.float64)


def mesh(values, origin, du, dv, dw, nu, nv, nw, iso, slot):
    """Surface nets over the kept blocks of nu * nv * nw dense values (the tiles hold the same values at the same points):
    (vertices float32 [V, 3], quads uint32 [Q, 4], cells int64 [V], edges int64 [Q], holes) in the ABI's order."""
    iso = np.float64(iso)
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 4), np.uint32), np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
    if min(nu, nv, nw) < 2:
        return none
    nbu, nbv, nbw = lattice_blocks(nu, nv, nw)
    v = np.asarray(values).astype(np.float64).reshape(nw, nv, nu)
    with np.errstate(invalid="ignore"):
        inside = v < iso
    finite = np.isfinite(v)

    def corner(a, dx, dy, dz):
        return a[dz:nw - 1 + dz, dy:nv - 1 + dy, dx:nu - 1 + dx]

    offsets = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    n_in = sum(corner(inside, *o).astype(np.int64) for o in offsets)
    all_finite = np.logical_and.reduce([corner(finite, *o) for o in offsets])
    mixed = (n_in > 0) & (n_in < 8)
    # the slot of every cell's block, and its local index
    zz, yy, xx = np.meshgrid(np.arange(nw - 1), np.arange(nv - 1), np.arange(nu - 1), indexing="ij")
    cell_slot = np.asarray(slot, np.int64).reshape(nbw, nbv, nbu)[zz // B, yy // B, xx // B]
    local = ((zz % B) * B + yy % B) * B + xx % B
    kept = cell_slot >= 0
    active = mixed & all_finite & kept
    holes = int((mixed & ~all_finite & kept).sum())

    ck, cj, ci = np.nonzero(active)
    order = np.argsort(cell_slot[ck, cj, ci] * (B * B * B) + local[ck, cj, ci], kind="stable")
    ck, cj, ci = ck[order], cj[order], ci[order]
    V = len(ci)
    vid = np.full((nw, nv, nu), -1, np.int64)
    vid[ck, cj, ci] = np.arange(V)
    cells = ((ck * nv + cj) * nu + ci).astype(np.int64)

    o, u, vv, w = _vectors(origin, du, dv, dw)
    sums = [np.zeros(V, np.float64) for _ in range(3)]
    m = np.zeros(V, np.int64)
    with np.errstate(all="ignore"):
        for A, off in EDGES:
            hi = list(off)
            hi[A] = 1
            a = v[ck + off[2], cj + off[1], ci + off[0]]
            b = v[ck + hi[2], cj + hi[1], ci + hi[0]]
            cross = (a < iso) != (b < iso)
            t = (iso - a) / (b - a)
            for c in range(3):
                add = t if c == A else np.float64(off[c])
                sums[c] = np.where(cross, sums[c] + add, sums[c])
            m = m + cross
        cnt = m.astype(np.float64)
        f = [s / cnt for s in sums]
        fi, fj, fk = ci.astype(np.float64) + f[0], cj.astype(np.float64) + f[1], ck.astype(np.float64) + f[2]
        vertices = np.empty((V, 3), np.float32)
        for c in range(3):
            s = o[c] + fi * u[c]
            s = s + fj * vv[c]
            s = s + fk * w[c]
            vertices[:, c] = s.astype(np.float32)

    n = (nu, nv, nw)
    keys, rows, edge_keys = [], [], []
    for A in range(3):
        Bx, Cx = CYCLIC[A]
        lo = [0, 0, 0]
        lo[Bx] = lo[Cx] = 1
        sl = tuple(slice(lo[ax], n[ax] - 1) for ax in (2, 1, 0))
        e = [np.zeros(3, np.int64) for _ in range(3)]
        for ax in range(3):
            e[ax][ax] = 1

        def shifted(arr, d):
            return arr[tuple(slice(lo[ax] + d[ax], n[ax] - 1 + d[ax]) for ax in (2, 1, 0))]

        differ = inside[sl] != shifted(inside, e[A])
        c0, c1, c2, c3 = shifted(vid, -e[Bx] - e[Cx]), shifted(vid, -e[Cx]), vid[sl], shifted(vid, -e[Bx])
        emit = differ & (c0 >= 0) & (c1 >= 0) & (c2 >= 0) & (c3 >= 0)
        pk, pj, pi = np.nonzero(emit)
        if not len(pi):
            continue
        p_in = inside[sl][pk, pj, pi]
        q = np.stack([c0[pk, pj, pi], np.where(p_in, c1[pk, pj, pi], c3[pk, pj, pi]), c2[pk, pj, pi],
                      np.where(p_in, c3[pk, pj, pi], c1[pk, pj, pi])], axis=1)
        gk, gj, gi = pk + lo[2], pj + lo[1], pi + lo[0]
        l = (gk * nv + gj) * nu + gi
        keys.append(cell_slot[gk, gj, gi] * (3 * B * B * B) + 3 * local[gk, gj, gi] + A)
        edge_keys.append(3 * l + A)
        rows.append(q)
    if not rows:
        return vertices, np.zeros((0, 4), np.uint32), cells, np.zeros(0, np.int64), holes
    keys, rows, edge_keys = np.concatenate(keys), np.concatenate(rows), np.concatenate(edge_keys)
    order = np.argsort(keys, kind="stable")
    return vertices, rows[order].astype(np.uint32), cells, edge_keys[order].astype(np.int64), holes


def sort_dense(vertices, quads, cells, edges):
    """The tile-ordered mesh in the dense mesher's order: vertices by cells, quads by edges, the vertices renamed."""
    by_cell = np.argsort(cells, kind="stable")
    rename = np.empty(len(cells), np.int64)
    rename[by_cell] = np.arange(len(cells))
    q = np.asarray(quads, np.int64)[np.argsort(edges, kind="stable")]
    return np.ascontiguousarray(vertices[by_cell]), (rename[q] if len(q) else q).astype(np.uint32).reshape(-1, 4)
