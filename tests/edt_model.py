"""A numpy restatement of the distance rule of include/rm_raymarch.h ("distances"), taking nothing from the library: the
set on one side of iso (parts_model.in_set), and for every point of it the squared index distance to the nearest lattice point
that is not in it.  Three axis passes of the direct min-plus out[a] = min over b of g[b] + (a - b)^2, RM_EDT_FAR an absent
term, in int64; everything is an integer and is compared for equality."""
import numpy as np

from parts_model import in_set  # noqa: F401  (the set's rule is the parts')

FAR = 2 ** 31 - 1  # RM_EDT_FAR


def min_plus(g, axis):
    """out[.., a, ..] = min over b with g[.., b, ..] != FAR of g[.., b, ..] + (a - b)^2 along `axis`; FAR where no such b."""
    g = np.moveaxis(np.asarray(g, np.int64), axis, -1)
    m = g.shape[-1]
    out = np.full(g.shape, FAR, np.int64)
    a = np.arange(m, dtype=np.int64)
    for b in range(m):
        term = np.where(g[..., b:b + 1] == FAR, FAR, g[..., b:b + 1] + (a - b) ** 2)
        out = np.minimum(out, term)
    return np.moveaxis(out, -1, axis)


def edt(s):
    """int32 [nw, nv, nu]: 0 outside S; inside, the squared index distance to the nearest point of the lattice outside S;
    FAR everywhere where S is the whole lattice."""
    s = np.asarray(s, bool)
    g = np.where(s, FAR, 0).astype(np.int64)
    for axis in (2, 1, 0):  # along i, j, k
        g = min_plus(g, axis)
    assert g.size == 0 or (g.min() >= 0 and g.max() <= FAR)
    return g.astype(np.int32)


def info(s, d2):
    s = np.asarray(s, bool)
    flat = np.asarray(d2).reshape(-1).astype(np.int64)
    if not s.any():
        return dict(n_points=int(s.size), n_set=0, max_d2=0, argmax=-1)
    most = int(flat[s.reshape(-1)].max())
    return dict(n_points=int(s.size), n_set=int(s.sum()), max_d2=most, argmax=int(np.flatnonzero(s.reshape(-1) & (flat == most))[0]))


def eroded(s, d2, r2):
    """The volume Edt.eroded returns: -1.0 where the point is in S and d2 >= r2, +1.0 elsewhere."""
    return np.where(np.asarray(s, bool) & (np.asarray(d2) >= r2), -1.0, 1.0)


def opened(s, r2):
    """The opening of S by the squared radius r2 as a -1 / +1 volume: erode, then every point closer than r2 to the eroded set."""
    s = np.asarray(s, bool)
    kept = eroded(s, edt(s), r2) < 0
    back = edt(~kept)  # over the complement of the eroded set: the squared distance to it
    return np.where(kept | (back < r2), -1.0, 1.0)


def max_by_part(d2, labels):
    """int64 [n_parts]: the largest d2 over each part of `labels` (parts_model.label's numbering)."""
    labels = np.asarray(labels).reshape(-1)
    n_parts = int(labels.max()) + 1 if labels.size and labels.max() >= 0 else 0
    d = np.asarray(d2).reshape(-1).astype(np.int64)
    return np.array([d[labels == p].max() for p in range(n_parts)], np.int64).reshape(n_parts)
