"""A numpy restatement of the two rules of the field queries in include/rm_raymarch.h, taking nothing from the library: the
points of a lattice (rm_lattice_points, field_kernel) as explicit float64 elementwise operations with one rounding to
float32, and the two colour rules of rm_shade_field in integer numpy."""
import numpy as np


def indices(nu, nv, nw, first=0, n=None):
    """(i, j, k) of the linear indices [first, first + n): l = (k * nv + j) * nu + i."""
    total = int(nu) * int(nv) * int(nw)
    n = total - first if n is None else n
    assert 0 <= first and 0 <= n and first + n <= total
    l = np.arange(first, first + n, dtype=np.int64)
    row = l // max(nu, 1)
    return l - row * nu, row % max(nv, 1), row // max(nv, 1)


def points(origin, du, dv, dw, nu, nv, nw, first=0, n=None):
    """float32 [n, 3]: component c of point (i, j, k) is f32(((origin[c] + i * du[c]) + j * dv[c]) + k * dw[c]), the vectors
    taken as float32 and widened, the products and sums in float64, left to right, one operation at a time."""
    o, u, v, w = (np.asarray(x, np.float32).astype(np.float64) for x in (origin, du, dv, dw))
    i, j, k = (x.astype(np.float64) for x in indices(nu, nv, nw, first, n))
    out = np.empty((len(i), 3), np.float32)
    with np.errstate(all="ignore"):
        for c in range(3):
            pi = i * u[c]
            pj = j * v[c]
            pk = k * w[c]
            s = o[c] + pi
            s = s + pj
            s = s + pk
            out[:, c] = s.astype(np.float32)
    return out


INSIDE, OUTSIDE = (60, 120, 230), (230, 140, 50)


def shade_distance(d, range=2.0, band=0.25, line=0.02):
    """uint8 [n, 4] for float64 distances: NaN magenta; |d| < line white; else intensity 96 + 159 * s // 255 with
    s = 255 from |d| / range >= 1, else trunc(|d| / range * 255.0); a quarter darker where trunc(|d| / band) is odd (0 from
    2^31 on); blue for d < 0, orange otherwise (-0.0 too).  Two float64 quotients, integers after them."""
    d = np.asarray(d, np.float64).reshape(-1)
    a = np.abs(d)
    nan = np.isnan(d)
    with np.errstate(all="ignore"):
        x = a / np.float64(range)
        y = a / np.float64(band)
        sat = x >= 1.0
        s = np.where(sat, 255, np.where(sat | nan, 0.0, x * 255.0).astype(np.int64))
        q = np.where(y < 2147483648.0, y, 0.0).astype(np.int64)
    I = 96 + 159 * s // 255
    I = np.where(q & 1, I * 3 // 4, I)
    base = np.where((d < 0.0)[:, None], np.array(INSIDE, np.int64), np.array(OUTSIDE, np.int64))
    rgb = base * I[:, None] // 255
    rgb[~nan & (a < line)] = 255
    rgb[nan] = (255, 0, 255)
    out = np.full((len(d), 4), 255, np.uint8)
    out[:, :3] = rgb
    return out


def shade_count(v, lo, hi):
    """uint8 [n, 4] for uint32 counts: s = 0 for v <= lo, 255 for v >= hi (in that order), else (v - lo) * 255 // (hi - lo);
    R = min(2s, 255), G = min(512 - 2s, 255), B = 0."""
    v = np.asarray(v).astype(np.int64).reshape(-1)
    lo, hi = int(lo), int(hi)
    s = np.where(v <= lo, 0, np.where(v >= hi, 255, (v - lo) * 255 // max(hi - lo, 1)))
    out = np.full((len(v), 4), 255, np.uint8)
    out[:, 0] = np.minimum(2 * s, 255)
    out[:, 1] = np.minimum(512 - 2 * s, 255)
    out[:, 2] = 0
    return out
