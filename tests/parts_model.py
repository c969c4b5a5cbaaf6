"""A numpy restatement of the parts rule of include/rm_raymarch.h ("parts"), taking nothing from the library: the set on one
side of iso, its 6-connected components numbered by their smallest linear index, and an rm_measure per component.  Labels,
counts and sums are integers, so everything is compared for equality."""
import numpy as np

from measure_model import INT32_MAX, Sums

SHARED = ("n_inside", "sum1", "sum2", "crossings", "lo", "hi")  # what the records' sum shares with rm_measure_field_device's


def in_set(values, nu, nv, nw, iso, side=0):
    """S as a bool array [nw, nv, nu]: side 0 value < iso (NaN and equality outside), side 1 the complement."""
    v = np.asarray(values).astype(np.float64).reshape(nw, nv, nu)
    with np.errstate(invalid="ignore"):
        inside = v < np.float64(iso)
    return ~inside if side else inside


def label(s):
    """int32 [nw, nv, nu]: the number of the 6-connected component of S a point lies in, or -1; components numbered in
    ascending order of their smallest linear index.  Every point of S takes the smallest root among itself and its
    neighbours in S, roots are followed to roots, until nothing changes: a root is then its component's smallest index."""
    s = np.asarray(s, bool)
    n = s.size
    none = np.int64(n)
    parent = np.where(s, np.arange(n, dtype=np.int64).reshape(s.shape), none)
    while True:
        least = parent.copy()
        for axis in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            least[lo] = np.minimum(least[lo], parent[hi])
            least[hi] = np.minimum(least[hi], parent[lo])
        least = np.where(s, least, none)
        # hook every point's root below what the point saw, then jump pointers to a fixed point
        flat = np.append(parent.reshape(-1), none)
        want = least.reshape(-1)
        np.minimum.at(flat, flat[:-1], want)
        flat[:-1] = np.minimum(flat[:-1], want)
        while True:
            jumped = flat[flat]
            if (jumped == flat).all():
                break
            flat = jumped
        new = np.where(s, flat[:-1].reshape(s.shape), none)
        if (new == parent).all():
            break
        parent = new
    roots = parent.reshape(-1)
    is_root = roots == np.arange(n)
    number = np.full(n + 1, -1, np.int64)
    number[:-1][is_root] = np.arange(int(is_root.sum()))
    return number[roots].reshape(s.shape).astype(np.int32)


def info(s, labels):
    return dict(n_points=int(s.size), n_set=int(s.sum()), n_parts=int(labels.max()) + 1 if s.any() else 0, gave_up=0)


def part_records(labels, n_records):
    """The first n_records records as dicts of measure_model's fields: over the points with label p; crossings[A] the lattice
    edges along A with exactly one end in S, for the part of the end in S.  Records beyond the parts are empty."""
    labels = np.asarray(labels)
    nw, nv, nu = labels.shape
    s = labels >= 0
    n_parts = int(labels.max()) + 1 if s.any() else 0
    count = min(n_parts, n_records)
    sums = [Sums() for _ in range(n_records)]
    if count:
        order = np.argsort(labels.reshape(-1), kind="stable")
        sorted_labels = labels.reshape(-1)[order]
        first = np.searchsorted(sorted_labels, np.arange(count + 1))
        for p in range(count):
            l = order[first[p]:first[p + 1]].astype(np.int64)
            sums[p].add_points(l % nu, (l // nu) % nv, l // (nu * nv))
        for axis, c in ((2, 0), (1, 1), (0, 2)):  # array axis -> lattice axis
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            a, b = labels[tuple(lo)], labels[tuple(hi)]
            owner = np.where((a >= 0) & (b < 0), a, np.where((b >= 0) & (a < 0), b, -1))
            per_part = np.bincount(owner[(owner >= 0) & (owner < count)], minlength=count)
            for p in range(count):
                sums[p].crossings[c] = int(per_part[p])
    return [x.record(nu * nv * nw) for x in sums]


def sum_records(records):
    """The records added field by field, the boxes united: the SHARED fields as a dict."""
    out = dict(n_inside=0, sum1=(0, 0, 0), sum2=(0,) * 6, crossings=(0, 0, 0), lo=(INT32_MAX,) * 3, hi=(-1,) * 3)
    for r in records:
        out["n_inside"] += r["n_inside"]
        for f in ("sum1", "sum2", "crossings"):
            out[f] = tuple(x + y for x, y in zip(out[f], r[f]))
        out["lo"] = tuple(min(x, y) for x, y in zip(out["lo"], r["lo"]))
        out["hi"] = tuple(max(x, y) for x, y in zip(out["hi"], r["hi"]))
    return out
