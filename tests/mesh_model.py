"""A numpy restatement of the surface-nets rule of include/rm_raymarch.h ("meshes"), taking nothing from the library: the
inside test, active cells and holes, the vertex numbering, the vertex position as explicit float64 elementwise operations in
the stated order with one rounding to float32, the quads with their winding and their order.  Vectorised over cells and
edges: the only Python loops run over the twelve edges of a cell and the three axes."""
import numpy as np

# the twelve cell edges in the rule's order: (axis A, offsets of the low corner as (dx, dy, dz)); within an axis the other two
# axes take (0,0), (1,0), (0,1), (1,1), the lower-numbered one first
EDGES = []
for _A in range(3):
    _lo, _hi = [x for x in range(3) if x != _A]
    for _o_lo, _o_hi in ((0, 0), (1, 0), (0, 1), (1, 1)):
        _off = [0, 0, 0]
        _off[_lo], _off[_hi] = _o_lo, _o_hi
        EDGES.append((_A, tuple(_off)))
CYCLIC = {0: (1, 2), 1: (2, 0), 2: (0, 1)}  # A -> (B, C)


def mesh(values, origin, du, dv, dw, nu, nv, nw, iso=0.0):
    """(vertices float32 [V, 3], quads uint32 [Q, 4], holes) for nu * nv * nw values in the lattice's linear order
    l = (k * nv + j) * nu + i (float64, or float32: widened)."""
    iso = np.float64(iso)
    none = np.zeros((0, 3), np.float32), np.zeros((0, 4), np.uint32), 0
    if min(nu, nv, nw) < 2:
        return none
    v = np.asarray(values).astype(np.float64).reshape(nw, nv, nu)
    with np.errstate(invalid="ignore"):
        inside = v < iso  # NaN: False
    finite = np.isfinite(v)

    def corner(a, dx, dy, dz):  # the cells' corner (dx, dy, dz) of a per-point array, indexed [k, j, i] by the low corner
        return a[dz:nw - 1 + dz, dy:nv - 1 + dy, dx:nu - 1 + dx]

    offsets = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    n_in = sum(corner(inside, *o).astype(np.int64) for o in offsets)
    all_finite = np.logical_and.reduce([corner(finite, *o) for o in offsets])
    mixed = (n_in > 0) & (n_in < 8)
    active = mixed & all_finite
    holes = int((mixed & ~all_finite).sum())

    # vertex numbers: active cells by the linear index of their low corner = C order of the [k, j, i] cell array
    vid = np.full((nw, nv, nu), -1, np.int64)  # per POINT: the vertex of the cell whose low corner it is, -1 without one
    ck, cj, ci = np.nonzero(active)
    V = len(ci)
    vid[ck, cj, ci] = np.arange(V)

    # positions
    o, u, vv, w = (np.asarray(x, np.float32).astype(np.float64) for x in (origin, du, dv, dw))
    sums = [np.zeros(V, np.float64) for _ in range(3)]
    m = np.zeros(V, np.int64)
    with np.errstate(all="ignore"):
        for A, off in EDGES:
            hi = list(off)
            hi[A] = 1
            a = v[ck + off[2], cj + off[1], ci + off[0]]
            b = v[ck + hi[2], cj + hi[1], ci + hi[0]]
            cross = (a < iso) != (b < iso)
            num = iso - a
            den = b - a
            t = num / den
            for c in range(3):
                add = t if c == A else np.float64(off[c])
                sums[c] = np.where(cross, sums[c] + add, sums[c])
            m = m + cross
        cnt = m.astype(np.float64)
        f = [s / cnt for s in sums]
        fi = ci.astype(np.float64) + f[0]
        fj = cj.astype(np.float64) + f[1]
        fk = ck.astype(np.float64) + f[2]
        vertices = np.empty((V, 3), np.float32)
        for c in range(3):
            pi = fi * u[c]
            pj = fj * vv[c]
            pk = fk * w[c]
            s = o[c] + pi
            s = s + pj
            s = s + pk
            vertices[:, c] = s.astype(np.float32)

    # quads: per axis the edges p -> p + e_A that change side and whose four cells exist and are active
    n = (nu, nv, nw)
    keys, rows = [], []
    for A in range(3):
        B, C = CYCLIC[A]
        lo = [0, 0, 0]
        lo[B] = lo[C] = 1  # p - e_B and p - e_C exist; every axis stops at n - 2: the cells at p, p - e_B, p - e_C, p - e_B - e_C exist
        sl = tuple(slice(lo[ax], n[ax] - 1) for ax in (2, 1, 0))  # [k, j, i]
        e = [np.zeros(3, np.int64) for _ in range(3)]
        for ax in range(3):
            e[ax][ax] = 1

        def shifted(arr, d):  # arr at p + d for every p of the region
            return arr[tuple(slice(lo[ax] + d[ax], n[ax] - 1 + d[ax]) for ax in (2, 1, 0))]

        differ = inside[sl] != shifted(inside, e[A])
        c0, c1, c2, c3 = shifted(vid, -e[B] - e[C]), shifted(vid, -e[C]), vid[sl], shifted(vid, -e[B])
        emit = differ & (c0 >= 0) & (c1 >= 0) & (c2 >= 0) & (c3 >= 0)
        pk, pj, pi = np.nonzero(emit)
        if not len(pi):
            continue
        p_in = inside[sl][pk, pj, pi]
        q = np.stack([c0[pk, pj, pi], np.where(p_in, c1[pk, pj, pi], c3[pk, pj, pi]), c2[pk, pj, pi],
                      np.where(p_in, c3[pk, pj, pi], c1[pk, pj, pi])], axis=1)
        l = ((pk + lo[2]) * nv + (pj + lo[1])) * nu + (pi + lo[0])
        keys.append(3 * l + A)
        rows.append(q)
    if not rows:
        return vertices, np.zeros((0, 4), np.uint32), holes
    keys, rows = np.concatenate(keys), np.concatenate(rows)
    order = np.argsort(keys, kind="stable")
    return vertices, rows[order].astype(np.uint32), holes


def edge_use(quads):
    """{undirected mesh edge: how many quads use it}."""
    q = np.asarray(quads, np.int64)
    e = np.concatenate([np.stack([q[:, s], q[:, (s + 1) % 4]], axis=1) for s in range(4)])
    e.sort(axis=1)
    uniq, counts = np.unique(e, axis=0, return_counts=True)
    return uniq, counts


def is_closed_manifold(quads):
    """Every edge is shared by exactly two quads and no quad names a vertex twice."""
    q = np.asarray(quads, np.int64)
    if not len(q):
        return False
    s = np.sort(q, axis=1)
    if (s[:, 1:] == s[:, :-1]).any():
        return False
    _, counts = edge_use(q)
    return bool((counts == 2).all())
