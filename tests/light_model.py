"""An independent numpy model of the light query's spawn arithmetic (include/rm_raymarch.h, rm_ray_light, steps 3-5) and of
the one line rm_shade_lit changes in PhongModel.shade.  It holds no marcher and no distance function: the tests feed it
distances and march results from entries that are pinned elsewhere (rm_ray_march, rm_scene_distance, the CPU oracle)."""
import numpy as np

MAX_DIST = 10.0


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def phong_light():
    """phongModel.ts:15-16: vec3.normalize of the Float32Array (1, -1, 1.5)."""
    v = np.array([1.0, -1.0, 1.5], np.float32).astype(np.float64)
    ln = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if ln > 0:
        ln = 1 / np.sqrt(ln)
    return f32(v * ln)


def scale_and_add(a, b, s):
    """vec3.scaleAndAdd into a Float32Array: f32(a + b * s) per component, one product and one sum in binary64."""
    s = np.asarray(s, np.float64)
    return f32(a.astype(np.float64) + b.astype(np.float64) * (s[..., None] if s.ndim else s))


def classify(t, normal, L):
    """neutral: t >= 10 or a zero normal.  c = n . L left to right in binary64; cast: a hit with c > 0 (NaN: not cast)."""
    n = normal.astype(np.float64)
    Ld = np.asarray(L, np.float32).astype(np.float64)
    neutral = (t >= MAX_DIST) | ((normal[:, 0] == 0) & (normal[:, 1] == 0) & (normal[:, 2] == 0))
    c = n[:, 0] * Ld[0] + n[:, 1] * Ld[1] + n[:, 2] * Ld[2]
    cast = ~neutral & (c > 0)
    return neutral, c, cast


def hit_points(origins, dirs, t):
    return scale_and_add(origins, dirs, t)


def shadow_origins(p, normal, bias):
    return scale_and_add(p, normal, float(bias))


def ao_points(p, normal, k, ao_step):
    """q_k = f32(p + n * h_k), h_k = k * ao_step."""
    return scale_and_add(p, normal, float(k) * float(ao_step))


def ao_value(d, ao_step, ao_strength):
    """d: [K, m] distances at the sample points -> float32[m].  occ summed in order of increasing k in binary64."""
    d = np.asarray(d, np.float64)
    occ = np.zeros(d.shape[1], np.float64)
    for k in range(1, d.shape[0] + 1):
        h = float(k) * float(ao_step)
        occ = occ + (h - d[k - 1]) * 2.0 ** (1 - k)
    x = 1.0 - float(ao_strength) * occ
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.where(x > 1, 1.0, x), 0.0).astype(np.float32)


def compose(origins, dirs, primary, L, bias, K, ao_step, ao_strength, march, distance):
    """The eight outputs of rm_ray_light from its rule.  primary = (t, iters, sdf, normal) of the rays with normals;
    march(o, d) -> (t, iters, sdf) of rays without normals; distance(points) -> (dist, count)."""
    t, iters, sdf, normal = primary
    n = len(t)
    neutral, c, cast = classify(t, normal, L)
    hit = ~neutral
    lit = np.ones(n, np.float32)
    ao = np.ones(n, np.float32)
    iters2 = np.zeros(n, np.uint32)
    sdf2 = np.zeros(n, np.uint32)
    p = hit_points(origins, dirs, t)
    lit[hit & ~cast] = 0
    if cast.any():
        so = shadow_origins(p[cast], normal[cast], bias)
        sd = np.ascontiguousarray(np.broadcast_to(np.asarray(L, np.float32), so.shape))
        ts, its, cs = march(so, sd)
        lit[cast] = np.where(ts >= MAX_DIST, 1, 0)
        iters2[cast] = its
        sdf2[cast] = cs
    if hit.any() and K > 0:
        ds = []
        for k in range(1, K + 1):
            d, cnt = distance(ao_points(p[hit], normal[hit], k, ao_step))
            ds.append(d)
            sdf2[hit] += cnt.astype(np.uint32)
        ao[hit] = ao_value(np.array(ds), ao_step, ao_strength)
    return t, iters, sdf, normal, lit, ao, iters2, sdf2


def shade_lit(depth, normal, lit, ao, L=None):
    """PhongModel.shade (phongModel.ts:33-72) with I = min((0.1 + diff s + spec s) a, 1) -> uint8 [n, 4].  pow is numpy's:
    the bytes agree with the device within 1 LSB, exactly where spec * s is 0."""
    Ld = (phong_light() if L is None else np.asarray(L, np.float32)).astype(np.float64)
    depth = np.asarray(depth, np.uint8).reshape(-1)
    nb = np.asarray(normal, np.uint8).reshape(-1, 3)
    n = f32(nb.astype(np.float64) / 127.5 - 1.0)
    nd = n.astype(np.float64)
    ln = nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1] + nd[:, 2] * nd[:, 2]
    with np.errstate(divide="ignore"):
        ln = np.where(ln > 0, 1 / np.sqrt(ln), ln)
    n = f32(nd * ln[:, None])
    nd = n.astype(np.float64)
    ndl = nd[:, 0] * Ld[0] + nd[:, 1] * Ld[1] + nd[:, 2] * Ld[2]
    diff = np.where(ndl > 0, ndl, 0.0)
    r = f32(nd * (2 * ndl)[:, None])
    r = f32(r.astype(np.float64) - Ld[None, :])
    rd = r.astype(np.float64)
    rl = rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1] + rd[:, 2] * rd[:, 2]
    with np.errstate(divide="ignore"):
        rl = np.where(rl > 0, 1 / np.sqrt(rl), rl)
    vdr = f32(rd[:, 2] * rl).astype(np.float64)
    spec = 0.5 * np.where(vdr > 0, vdr, 0.0) ** 32
    s = np.asarray(lit, np.float32).astype(np.float64).reshape(-1)
    a = np.asarray(ao, np.float32).astype(np.float64).reshape(-1)
    inten = np.minimum((0.1 + diff * s + spec * s) * a, 1.0)
    color = 255 * inten * (1 - depth.astype(np.float64) / 255)
    c = np.where(color > 0, np.where(color >= 255, 255.0, np.rint(color)), 0.0).astype(np.uint8)
    out = np.stack([c, c, c, np.full_like(c, 255)], axis=1)
    out[depth >= 255] = (10, 10, 20, 255)
    return out
