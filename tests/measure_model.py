"""A numpy restatement of the measure rule of include/rm_raymarch.h ("measures"), taking nothing from the library: the dense
record over nu * nv * nw values, the sparse record over the tiles of the kept blocks plus the dropped blocks that lie inside,
and the conversion to world units.  Everything measured is an integer, so the records are compared for equality; `world`
follows the header's order of operations in Python floats (binary64, one operation at a time) and is compared bit for bit.
The coarse decision -- centres, bound, blocks, tile_indices, tiles -- is tests/mesh_sparse_model.py's, not restated here."""
import math

import numpy as np

from mesh_sparse_model import B, lattice_blocks

INT32_MAX = 2 ** 31 - 1
FIELDS = ("n_points", "n_inside", "n_nonfinite", "sum1", "sum2", "crossings", "lo", "hi", "n_blocks", "n_kept", "n_blocks_inside")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))  # sum2's order, and second's


class Sums:
    """The running integer sums of a record (Python ints: no overflow to think about)."""

    def __init__(self):
        self.n_inside = self.n_nonfinite = self.n_blocks_inside = 0
        self.sum1, self.sum2, self.crossings = [0, 0, 0], [0] * 6, [0, 0, 0]
        self.lo, self.hi = [INT32_MAX] * 3, [-1] * 3

    def add_points(self, i, j, k):
        """Inside points at the int64 index arrays i, j, k."""
        if not len(i):
            return
        idx = (i, j, k)
        self.n_inside += len(i)
        for c in range(3):
            self.sum1[c] += int(idx[c].sum())
            self.lo[c] = min(self.lo[c], int(idx[c].min()))
            self.hi[c] = max(self.hi[c], int(idx[c].max()))
        for e, (a, b) in enumerate(PAIRS):
            self.sum2[e] += int((idx[a] * idx[b]).sum())

    def record(self, n_points, n_blocks=0, n_kept=0):
        return dict(n_points=n_points, n_inside=self.n_inside, n_nonfinite=self.n_nonfinite, sum1=tuple(self.sum1), sum2=tuple(self.sum2),
                    crossings=tuple(self.crossings), lo=tuple(self.lo), hi=tuple(self.hi), n_blocks=n_blocks, n_kept=n_kept,
                    n_blocks_inside=self.n_blocks_inside)


def measure_dense(values, nu, nv, nw, iso):
    """rm_measure_field_device's record as a dict of Python ints (tuples for the arrays), keys FIELDS."""
    s = Sums()
    v = np.asarray(values).astype(np.float64).reshape(nw, nv, nu)
    with np.errstate(invalid="ignore"):
        inside = v < np.float64(iso)
    s.n_nonfinite = int((~np.isfinite(v)).sum())
    k, j, i = (x.astype(np.int64) for x in np.nonzero(inside))
    s.add_points(i, j, k)
    s.crossings = [int((inside[:, :, 1:] != inside[:, :, :-1]).sum()), int((inside[:, 1:, :] != inside[:, :-1, :]).sum()),
                   int((inside[1:, :, :] != inside[:-1, :, :]).sum())]
    return s.record(nu * nv * nw)


def owned(n, nb, b):
    """The lattice points block b of an axis with n points and nb blocks owns: 8 b .. 8 b + 7, and the last block point 8 nb
    too when that index is <= n - 1 -- clipped to the lattice."""
    last = B * b + B - 1 + (1 if b == nb - 1 and B * nb <= n - 1 else 0)
    return np.arange(B * b, min(last, n - 1) + 1, dtype=np.int64)


def measure_sparse(tiles, slot, lst, dist, nu, nv, nw, iso):
    """rm_measure_tiles_device's record from tiles float64 [n_kept, 729], slot int32 [n_blocks], lst int32 [n_kept] and the
    distances at the block centres: kept blocks from their tile values, dropped ones with dist - iso < 0 wholly inside."""
    s = Sums()
    iso = np.float64(iso)
    n = (nu, nv, nw)
    nb = lattice_blocks(nu, nv, nw)
    n_blocks = nb[0] * nb[1] * nb[2]
    tiles = np.asarray(tiles, np.float64).reshape(-1, 9, 9, 9)  # [slot, g, b, a]
    for b in range(n_blocks):
        bc = (b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1]))
        own = [owned(n[c], nb[c], bc[c]) for c in range(3)]
        k, j, i = (x.reshape(-1) for x in np.meshgrid(own[2], own[1], own[0], indexing="ij"))
        if slot[b] < 0:
            if np.float64(dist[b]) - iso < 0:
                s.add_points(i, j, k)
                s.n_blocks_inside += 1
            continue
        t = tiles[slot[b]]
        a, bb, g = i - B * bc[0], j - B * bc[1], k - B * bc[2]
        v = t[g, bb, a]
        with np.errstate(invalid="ignore"):
            inside = v < iso
            s.n_nonfinite += int((~np.isfinite(v)).sum())
            s.add_points(i[inside], j[inside], k[inside])
            # an edge belongs to the owner of its low end; it exists when its high end is a lattice point (by index)
            for c, (idx, off) in enumerate(((i, (0, 0, 1)), (j, (0, 1, 0)), (k, (1, 0, 0)))):
                has = idx + 1 < n[c]
                far = t[g[has] + off[0], bb[has] + off[1], a[has] + off[2]] < iso
                s.crossings[c] += int((far != inside[has]).sum())
    return s.record(nu * nv * nw, n_blocks, len(lst))


def same_measure(a, b, sparse_fields=False):
    """Two records equal field by field; the block fields and n_nonfinite only with sparse_fields."""
    apart = () if sparse_fields else ("n_blocks", "n_kept", "n_blocks_inside", "n_nonfinite")
    return all(a[f] == b[f] for f in FIELDS if f not in apart)


def world(lattice, record):
    """rm_measure_world: lattice = (origin, du, dv, dw) (rounded to binary32 first, as rm_lattice holds them), record a dict
    as above -> dict(cell_volume, volume, centroid, second, projected_area, area_estimate) of Python floats and tuples."""
    o, u, v, w = ([float(x) for x in np.asarray(vec, np.float32).reshape(3)] for vec in lattice)
    M = [[u[p], v[p], w[p]] for p in range(3)]  # M[p][a]: component p of step a
    cv = abs((u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0])) + u[2] * (v[0] * w[1] - v[1] * w[0]))
    n_inside = record["n_inside"]
    N = float(n_inside)
    S = [float(x) for x in record["sum1"]]
    nan = float("nan")
    m = [S[a] / N if n_inside else nan for a in range(3)]  # (0.0 / 0.0 in C)
    centroid = tuple(((o[c] + m[0] * M[c][0]) + m[1] * M[c][1]) + m[2] * M[c][2] for c in range(3))
    second = [0.0] * 6
    if n_inside:
        C = [[0.0] * 3 for _ in range(3)]
        for e, (a, b) in enumerate(PAIRS):
            C[a][b] = C[b][a] = float(record["sum2"][e]) - (S[a] * S[b]) / N
        for e, (p, q) in enumerate(PAIRS):
            t = [(C[a][0] * M[q][0] + C[a][1] * M[q][1]) + C[a][2] * M[q][2] for a in range(3)]
            pushed = (M[p][0] * t[0] + M[p][1] * t[1]) + M[p][2] * t[2]
            own = (M[p][0] * M[q][0] + M[p][1] * M[q][1]) + M[p][2] * M[q][2]
            second[e] = pushed * cv + ((N * cv) / 12.0) * own
    area = []
    for A in range(3):
        Bx, Cx = (A + 1) % 3, (A + 2) % 3
        x = M[1][Bx] * M[2][Cx] - M[2][Bx] * M[1][Cx]
        y = M[2][Bx] * M[0][Cx] - M[0][Bx] * M[2][Cx]
        z = M[0][Bx] * M[1][Cx] - M[1][Bx] * M[0][Cx]
        area.append(float(record["crossings"][A]) * math.sqrt((x * x + y * y) + z * z))
    return dict(cell_volume=cv, volume=N * cv, centroid=centroid, second=tuple(second), projected_area=tuple(area),
                area_estimate=(2.0 / 3.0) * ((area[0] + area[1]) + area[2]))
