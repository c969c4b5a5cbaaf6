"""A numpy model of rm_compare_frames, written from the definitions in include/rm_raymarch.h ("two renders of a view"), not
from the kernel: the expectation of tests/test_compare_frames.py and tests/test_napi_compare.py."""
import numpy as np

MAPS = {"none": -1, "sdf": 0, "iters": 1, "depth": 2, "normal": 3, "surface": 4}
FIELDS = ("pixels", "sum_sdf_a", "sum_sdf_b", "sum_iters_a", "sum_iters_b", "sum_abs_depth", "surface_a", "surface_b",
          "surface_only_a", "surface_only_b", "depth_differs", "normal_differs", "counters_differ", "b_cheaper", "a_cheaper",
          "max_abs_depth", "max_abs_normal")
ZERO = {name: 0 for name in FIELDS}


def _signed_map(a, b, gain):
    d = b.astype(np.int64) - a.astype(np.int64)
    m = np.minimum(np.abs(d) * gain, 255)
    out = np.zeros((d.size, 4), np.uint8)
    out[:, 0] = np.where(d > 0, m, 0)
    out[:, 1] = np.where(d < 0, m, 0)
    out[:, 3] = 255
    return out


def compare_frame(a, b, npx, map, gain):
    """One frame: a, b = (depth u8[npx], normal u8[3 npx], sdf u16[npx], iters u16[npx]) with None for an absent pair.
    -> (record dict, rgba u8[npx, 4] or None)."""
    (da, na, sa, ia), (db, nb, sb, ib) = a, b
    r = dict(ZERO, pixels=npx)
    if da is not None:
        dd = np.abs(db.astype(np.int64) - da.astype(np.int64))
        r["sum_abs_depth"], r["max_abs_depth"], r["depth_differs"] = int(dd.sum()), int(dd.max(initial=0)), int((dd != 0).sum())
    if na is not None:
        pa, pb = na.reshape(-1, 3), nb.reshape(-1, 3)
        surf_a, surf_b = (pa != 128).any(axis=1), (pb != 128).any(axis=1)
        dn = np.abs(pb.astype(np.int64) - pa.astype(np.int64)).max(axis=1, initial=0)
        r["surface_a"], r["surface_b"] = int(surf_a.sum()), int(surf_b.sum())
        r["surface_only_a"], r["surface_only_b"] = int((surf_a & ~surf_b).sum()), int((surf_b & ~surf_a).sum())
        r["normal_differs"], r["max_abs_normal"] = int((dn != 0).sum()), int(dn.max(initial=0))
    if sa is not None:
        r["sum_sdf_a"], r["sum_sdf_b"] = int(sa.astype(np.uint64).sum()), int(sb.astype(np.uint64).sum())
        r["b_cheaper"], r["a_cheaper"] = int((sb < sa).sum()), int((sa < sb).sum())
    if ia is not None:
        r["sum_iters_a"], r["sum_iters_b"] = int(ia.astype(np.uint64).sum()), int(ib.astype(np.uint64).sum())
    if sa is not None or ia is not None:
        differ = np.zeros(npx, bool)
        if sa is not None:
            differ |= sa != sb
        if ia is not None:
            differ |= ia != ib
        r["counters_differ"] = int(differ.sum())
    if map == MAPS["none"]:
        return r, None
    if map == MAPS["sdf"]:
        return r, _signed_map(sa, sb, gain)
    if map == MAPS["iters"]:
        return r, _signed_map(ia, ib, gain)
    if map == MAPS["depth"]:
        return r, _signed_map(da, db, gain)
    out = np.zeros((npx, 4), np.uint8)
    out[:, 3] = 255
    if map == MAPS["normal"]:
        out[:, 0] = out[:, 1] = np.minimum(dn * gain, 255)
    else:  # surface
        out[surf_a & surf_b, :3] = 96
        out[surf_b & ~surf_a, 0] = 255
        out[surf_a & ~surf_b, 1] = 255
    return r, out


def compare_frames(a, b, npx, n_frames, map, gain):
    """n_frames frames of npx pixels, one behind the other in every buffer -> (list of records, rgba u8[n_frames * npx * 4] or None)."""
    recs, imgs = [], []
    bpp = (1, 3, 1, 1)  # elements per pixel
    for k in range(n_frames):
        fa = tuple(None if x is None else x[k * npx * e:(k + 1) * npx * e] for x, e in zip(a, bpp))
        fb = tuple(None if x is None else x[k * npx * e:(k + 1) * npx * e] for x, e in zip(b, bpp))
        r, img = compare_frame(fa, fb, npx, map, gain)
        recs.append(r)
        imgs.append(img)
    if map == MAPS["none"]:
        return recs, None
    return recs, (np.concatenate(imgs).reshape(-1) if imgs else np.zeros(0, np.uint8))
