"""The rule of rm_scene_sharpen (include/rm_raymarch.h, "sharp meshes") restated in numpy over a distance callable, for tests:
the callable is D(points float32 [m, 3]) -> (dist float64 [m], count [m]) as in point_model.py (oracle_distance,
context_distance).  Every step is an explicit elementwise binary64 operation in the order the header states, with the one
rounding to binary32 where it says so; the loops run over corners, edges, refinement steps and Jacobi rotations, never over
vertices.  G(p, d) is point_model.gradient, the G of rm_scene_points."""
import collections

import numpy as np

from mesh_model import EDGES
from point_model import gradient

SharpResult = collections.namedtuple("SharpResult", "position feature count")

SWEEPS = 6
PAIRS = ((0, 1), (0, 2), (1, 2))


def lattice_point(origin, du, dv, dw, fi, fj, fk, rounded=True):
    """The lattice's point rule at the (fractional) binary64 indices fi, fj, fk -> [m, 3], float32 (one rounding) or float64."""
    o, u, v, w = (np.asarray(x, np.float32).astype(np.float64) for x in (origin, du, dv, dw))
    out = np.empty((len(fi), 3), np.float32 if rounded else np.float64)
    with np.errstate(all="ignore"):
        for c in range(3):
            s = o[c] + fi * u[c]
            s = s + fj * v[c]
            s = s + fk * w[c]
            out[:, c] = s.astype(np.float32) if rounded else s
    return out


def jacobi(a00, a01, a02, a11, a12, a22):
    """Six cyclic Jacobi sweeps over the symmetric 3 x 3 matrices -> (a [n, 3, 3] with the eigenvalues on the diagonal,
    V [n, 3, 3] with eigenvector i in column i)."""
    n = len(a00)
    a = np.empty((n, 3, 3), np.float64)
    a[:, 0, 0], a[:, 1, 1], a[:, 2, 2] = a00, a11, a22
    a[:, 0, 1] = a[:, 1, 0] = a01
    a[:, 0, 2] = a[:, 2, 0] = a02
    a[:, 1, 2] = a[:, 2, 1] = a12
    V = np.zeros((n, 3, 3), np.float64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                r = 3 - p - q
                apq = a[:, p, q].copy()
                go = ~(apq == 0)
                theta = (a[:, q, q] - a[:, p, p]) / (2 * apq)
                t = 1 / (np.abs(theta) + np.sqrt(theta * theta + 1))
                t = np.where(theta >= 0, t, -t)
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                h = t * apq
                app, aqq = a[:, p, p] - h, a[:, q, q] + h
                arp, arq = c * a[:, r, p] - s * a[:, r, q], s * a[:, r, p] + c * a[:, r, q]
                a[:, p, p] = np.where(go, app, a[:, p, p])
                a[:, q, q] = np.where(go, aqq, a[:, q, q])
                a[:, p, q] = a[:, q, p] = np.where(go, 0.0, apq)
                a[:, r, p] = a[:, p, r] = np.where(go, arp, a[:, r, p])
                a[:, r, q] = a[:, q, r] = np.where(go, arq, a[:, r, q])
                for k in range(3):
                    vp, vq = c * V[:, k, p] - s * V[:, k, q], s * V[:, k, p] + c * V[:, k, q]
                    V[:, k, p] = np.where(go, vp, V[:, k, p])
                    V[:, k, q] = np.where(go, vq, V[:, k, q])
    return a, V


def descending(lam):
    """The order of the eigenvalues [n, 3]: three compare-and-swap steps on (0, 1), (1, 2), (0, 1), a swap only when the later
    value is strictly greater -> idx [n, 3]."""
    n = len(lam)
    idx = np.tile(np.arange(3), (n, 1))
    rows = np.arange(n)
    with np.errstate(invalid="ignore"):
        for x, y in ((0, 1), (1, 2), (0, 1)):
            swap = lam[rows, idx[:, y]] > lam[rows, idx[:, x]]
            ix, iy = idx[:, x].copy(), idx[:, y].copy()
            idx[:, x] = np.where(swap, iy, ix)
            idx[:, y] = np.where(swap, ix, iy)
    return idx


def reach_radius(du, dv, dw):
    """rho: half the longest of the four body diagonals |du +- dv +- dw| of a cell."""
    u, v, w = (np.asarray(x, np.float32).astype(np.float64) for x in (du, dv, dw))
    longest = None
    for sv, sw in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        d = (u + v if sv > 0 else u - v)
        d = d + w if sw > 0 else d - w
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        if longest is None or length > longest:
            longest = length
    return 0.5 * longest


def lattice_values(D, origin, du, dv, dw, nu, nv, nw):
    """D at every point of the lattice, in its linear order -> float64 [nu * nv * nw]."""
    l = np.arange(nu * nv * nw)
    pts = lattice_point(origin, du, dv, dw, (l % nu).astype(np.float64), ((l // nu) % nv).astype(np.float64), (l // (nu * nv)).astype(np.float64))
    return D(pts)[0]


def active_cells(values, nu, nv, nw, iso=0.0):
    """The keys of the active cells of the meshers' rule in vertex order: all eight corners finite, neither all inside nor all
    outside -> int64 [V]."""
    v = np.asarray(values, np.float64).reshape(nw, nv, nu)
    with np.errstate(invalid="ignore"):
        inside = v < np.float64(iso)
    finite = np.isfinite(v)
    corners = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    cut = lambda a, dx, dy, dz: a[dz:nw - 1 + dz, dy:nv - 1 + dy, dx:nu - 1 + dx]  # noqa: E731
    n_in = sum(cut(inside, *c).astype(np.int64) for c in corners)
    ok = np.logical_and.reduce([cut(finite, *c) for c in corners])
    ck, cj, ci = np.nonzero((n_in > 0) & (n_in < 8) & ok)
    return ((ck * nv + cj) * nu + ci).astype(np.int64)


def sharpen(D, cells, origin, du, dv, dw, nu, nv, nw, iso=0.0, rank_tol=0.1, reach=1.0, refine=2):
    """The rule, every vertex at once: -> SharpResult(position float32 [n, 3], feature int32 [n], count uint64 [n])."""
    iso = np.float64(iso)
    l = np.asarray(cells, np.int64).reshape(-1)
    n = len(l)
    position = np.zeros((n, 3), np.float32)
    feature = np.full(n, -1, np.int32)
    count = np.zeros(n, np.uint64)
    in_range = (l >= 0) & (l < nu * nv * nw)
    ls = np.where(in_range, l, 0)
    row = ls // max(nu, 1)
    ci = ls - row * nu
    ck = row // max(nv, 1)
    cj = row - ck * nv
    exists = in_range & (ci + 1 < nu) & (cj + 1 < nv) & (ck + 1 < nw)
    vert = np.nonzero(exists)[0]  # everything below is indexed by position in `vert`
    m = len(vert)
    if not m:
        return SharpResult(position, feature, count)
    ci, cj, ck = ci[vert], cj[vert], ck[vert]
    lat = (origin, du, dv, dw)

    # 1. corners
    v = np.empty((m, 8), np.float64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        v[:, c], k = D(lattice_point(*lat, (ci + dx).astype(np.float64), (cj + dy).astype(np.float64), (ck + dz).astype(np.float64)))
        count[vert] += k.astype(np.uint64)
    with np.errstate(invalid="ignore"):
        inside = v < iso
    n_in = inside.sum(axis=1)
    active = np.isfinite(v).all(axis=1) & (n_in > 0) & (n_in < 8)
    half = np.float64(0.5)
    centre = lattice_point(*lat, ci.astype(np.float64) + half, cj.astype(np.float64) + half, ck.astype(np.float64) + half, rounded=False)
    position[vert] = centre.astype(np.float32)

    # 2. crossings, in (vertex, edge) order
    low = np.array([off[0] + 2 * off[1] + 4 * off[2] for _, off in EDGES])
    high = np.array([lo + (1 << A) for (A, _), lo in zip(EDGES, low)])
    cross = active[:, None] & (inside[:, low] != inside[:, high])
    xv, xe = np.nonzero(cross)
    nx = len(xv)
    rec = np.full((m, 12), -1, np.int64)
    rec[xv, xe] = np.arange(nx)
    a, b = v[xv, low[xe]], v[xv, high[xe]]
    axis = np.array([A for A, _ in EDGES])[xe]
    off = np.array([o for _, o in EDGES], np.int64)[xe]  # [nx, 3]
    base = [(c_[xv] + off[:, ax]).astype(np.float64) for ax, c_ in enumerate((ci, cj, ck))]
    tl, fl, th, fh = np.zeros(nx), a.copy(), np.ones(nx), b.copy()
    alive = np.ones(nx, bool)
    p = np.zeros((nx, 3), np.float32)
    d = np.zeros(nx, np.float64)
    xcount = np.zeros(nx, np.uint64)
    for it in range(refine + 1):
        with np.errstate(all="ignore"):
            t = tl + (iso - fl) * (th - tl) / (fh - fl)
            idx = [np.where(axis == ax, base[ax] + t, base[ax]) for ax in range(3)]
        p = lattice_point(*lat, *idx)
        alive &= np.isfinite(t) & np.isfinite(p).all(axis=1)
        at = np.nonzero(alive)[0]
        f = np.full(nx, np.nan)
        if len(at):
            f[at], k = D(p[at])
            xcount[at] += k.astype(np.uint64)
        if it == refine:
            d = f
            break
        with np.errstate(invalid="ignore"):
            same = (f < iso) == (a < iso)
        tl, fl = np.where(same, t, tl), np.where(same, f, fl)
        th, fh = np.where(same, th, t), np.where(same, fh, f)
    nrm = np.zeros((nx, 3), np.float32)
    at = np.nonzero(alive)[0]
    if len(at):
        nrm[at], k = gradient(D, p[at], d[at])
        xcount[at] += k.astype(np.uint64)
    keep = alive & np.isfinite(nrm).all(axis=1)
    np.add.at(count, vert[xv], xcount)

    # 3. quadric, in edge order
    P64, N64 = p.astype(np.float64), nrm.astype(np.float64)
    kept = np.zeros(m, np.int64)
    mean = np.zeros((m, 3), np.float64)
    sel = [(rec[:, e] >= 0) & keep[np.maximum(rec[:, e], 0)] for e in range(12)]
    for e in range(12):
        r = np.maximum(rec[:, e], 0)
        mean = np.where(sel[e][:, None], mean + P64[r], mean)
        kept += sel[e]
    with np.errstate(all="ignore"):
        mean = mean / kept.astype(np.float64)[:, None]
    A6 = np.zeros((m, 6), np.float64)
    bb = np.zeros((m, 3), np.float64)
    with np.errstate(all="ignore"):
        for e in range(12):
            r = np.maximum(rec[:, e], 0)
            nn, pp = N64[r], P64[r]
            prods = np.stack([nn[:, 0] * nn[:, 0], nn[:, 0] * nn[:, 1], nn[:, 0] * nn[:, 2], nn[:, 1] * nn[:, 1], nn[:, 1] * nn[:, 2],
                              nn[:, 2] * nn[:, 2]], axis=1)
            A6 = np.where(sel[e][:, None], A6 + prods, A6)
            s = (nn[:, 0] * (pp[:, 0] - mean[:, 0]) + nn[:, 1] * (pp[:, 1] - mean[:, 1])) + nn[:, 2] * (pp[:, 2] - mean[:, 2])
            bb = np.where(sel[e][:, None], bb + nn * s[:, None], bb)
    solve = active & (kept > 0)
    feature[vert[active]] = 0

    # 4. eigenvectors, 5. rank and reach
    if solve.any():
        sv = np.nonzero(solve)[0]
        am, V = jacobi(*(A6[sv, c] for c in range(6)))
        lam = np.stack([am[:, 0, 0], am[:, 1, 1], am[:, 2, 2]], axis=1)
        order = descending(lam)
        rows = np.arange(len(sv))
        lam = lam[rows[:, None], order]
        vec = [V[rows, :, order[:, i]] for i in range(3)]  # eigenvector i as [n, 3]
        with np.errstate(all="ignore"):
            lmax = lam[:, 0]
            r0 = np.where(lmax > 0, (lam > rank_tol * lmax[:, None]).sum(axis=1), 0)
            rho = reach_radius(du, dv, dw)
            limit = np.float64(reach) * rho
            coef = []
            for i in range(3):
                dot = (vec[i][:, 0] * bb[sv, 0] + vec[i][:, 1] * bb[sv, 1]) + vec[i][:, 2] * bb[sv, 2]
                coef.append(dot / lam[:, i])
            x = mean[sv].copy()
            rank = np.zeros(len(sv), np.int32)
            done = np.zeros(len(sv), bool)
            for r in (3, 2, 1):
                cand = mean[sv].copy()
                for i in range(r):
                    cand = cand + vec[i] * coef[i][:, None]
                dd = cand - centre[sv]
                dist = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
                take = ~done & (r0 >= r) & (dist <= limit)
                x = np.where(take[:, None], cand, x)
                rank = np.where(take, r, rank)
                done |= take
            position[vert[sv]] = x.astype(np.float32)
        feature[vert[sv]] = rank
    return SharpResult(position, feature, count)
