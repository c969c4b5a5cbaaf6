"""A numpy model of rm_counter_hist and rm_shade_ranged, written from the definitions in include/rm_raymarch.h ("counter
distributions per frame"), not from the kernels: the expectation of tests/test_counter_hist.py."""
import numpy as np

BINS = 256
MASKS = {"all": 0, "surface": 1, "background": 2}
FIELDS = ("pixels", "sum", "min", "max", "range_lo", "range_hi", "shift", "reserved")


def zero(shift):
    return dict({f: 0 for f in FIELDS}, shift=shift, bins=np.zeros(BINS, np.uint32))


def bin_of(p, bins, M):
    """b_p: r = floor(p (M - 1) / 1000), the smallest b with bins[0] + .. + bins[b] > r."""
    r = p * (M - 1) // 1000
    total = 0
    for b in range(BINS):
        total += int(bins[b])
        if total > r:
            return b
    raise AssertionError("the bins hold fewer than M pixels")


def counter_record(values, shift, lo_permille, hi_permille):
    """One rm_counter_hist of the selected values (u16 array) of one counter of one frame."""
    v = np.asarray(values, dtype=np.uint16).astype(np.int64)
    M = int(v.size)
    if M == 0:
        return zero(shift)
    bins = np.bincount(np.minimum(v >> shift, BINS - 1), minlength=BINS).astype(np.uint32)
    mn, mx = int(v.min()), int(v.max())
    b_lo, b_hi = bin_of(lo_permille, bins, M), bin_of(hi_permille, bins, M)
    return dict(pixels=M, sum=int(v.sum()), min=mn, max=mx, range_lo=max(mn, b_lo << shift),
                range_hi=mx if b_hi == BINS - 1 else min(mx, ((b_hi + 1) << shift) - 1), shift=shift, reserved=0, bins=bins)


def counter_hist(sdf, iters, normal, npx, n_frames, mask, shift, lo_permille, hi_permille):
    """n_frames frames of npx pixels, one behind the other in every buffer -> a list of {"sdf": record, "iters": record}."""
    out = []
    for k in range(n_frames):
        sel = np.ones(npx, bool)
        if mask != MASKS["all"]:
            surface = (normal[3 * k * npx:3 * (k + 1) * npx].reshape(-1, 3) != 128).any(axis=1)
            sel = surface if mask == MASKS["surface"] else ~surface
        frame = {}
        for name, buf in (("sdf", sdf), ("iters", iters)):
            frame[name] = zero(shift) if buf is None else counter_record(buf[k * npx:(k + 1) * npx][sel], shift, lo_permille, hi_permille)
        out.append(frame)
    return out


def shade_ranged(values, npx, n_frames, ranges):
    """ranges: one (lo, hi) per frame -> rgba u8[n_frames * npx * 4]."""
    out = np.zeros((n_frames * npx, 4), np.uint8)
    for k in range(n_frames):
        lo, hi = ranges[k]
        v = values[k * npx:(k + 1) * npx].astype(np.int64)
        s = np.where(v <= lo, 0, np.where(v >= hi, 255, (v - lo) * 255 // max(1, hi - lo)))
        out[k * npx:(k + 1) * npx, 0] = np.minimum(2 * s, 255)
        out[k * npx:(k + 1) * npx, 1] = np.minimum(512 - 2 * s, 255)
    out[:, 3] = 255
    return out.reshape(-1)


def same(a, b):
    """The fields in which two decoded records differ (empty: equal)."""
    bad = {f: (a[f], b[f]) for f in FIELDS if int(a[f]) != int(b[f])}
    if not np.array_equal(np.asarray(a["bins"], np.uint32), np.asarray(b["bins"], np.uint32)):
        bad["bins"] = np.nonzero(np.asarray(a["bins"], np.uint32) != np.asarray(b["bins"], np.uint32))[0][:8].tolist()
    return bad
