"""Light-query throughput (rm_ray_light_device, light_kernel<...>) against the ray query alone (rm_ray_march_device with
normals) and against the path a host had to compose before: primary march, spawn arithmetic in torch, a second march for the
shadow rays, and the occlusion samples through rm_scene_distance's host round trip.  One GPU.  Run each step under its own
time limit, e.g.

    timeout -k 10 300 python scripts/light_bench.py --case C3
    timeout -k 10 300 python scripts/light_bench.py --case C5
    timeout -k 10 300 python scripts/light_bench.py --case counts

C3 / C5: the rays of scripts/pick_bench.py.  light_ms and march_ms are HIP-event times of the call (median of --reps after
--warmup); composed_ms is wall time around the composed path with the device idle before and after (median of
--composed-reps; it crosses the host).  The eight outputs of the light query and of the composed path must hash alike, and so
must the four the light query shares with the ray query; the exit status is 1 otherwise.  counts: the secondary work per hit
ray -- shadow-ray iterations and SDF calls, occlusion-sample SDF calls -- of the 640 x 360 frame of C3's view under every
marcher and acceleration structure.  One JSON line per case (one per configuration for counts)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pick_bench import rays_c3, rays_c5  # noqa: E402
from ray_bench import timed  # noqa: E402

BIAS, K, AO_STEP, AO_STRENGTH = 0.02, 5, 0.05, 1.0  # Context.light's defaults
ALGS = ("sphere-tracer", "fixed-step", "adaptive-step", "adaptive-step-v2", "adaptive-step-v3")


def digest(arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).tobytes())
    return h.hexdigest()[:16]


def classes(t, nrm, L):
    """(hit, cast) of the rule: a hit has t < 10 and a non-zero normal; its shadow ray is cast when n . L > 0."""
    hit = (t < 10) & (nrm != 0).any(axis=1)
    nd, Ld = nrm.astype(np.float64), np.asarray(L, np.float32).astype(np.float64)
    return hit, hit & (nd[:, 0] * Ld[0] + nd[:, 1] * Ld[1] + nd[:, 2] * Ld[2] > 0)


def spawn(torch, a, b, s):
    """vec3.scaleAndAdd into a Float32Array: f32(a + b * s) in binary64."""
    return (a.double() + b.double() * s).float()


def composed(torch, ctx, og, dg, L):
    """What a host composed from rm_ray_march_device and rm_scene_distance before rm_ray_light: the same eight outputs."""
    t, it, sdf, nrm = ctx.ray_march(og, dg, normal=True)
    n = len(t)
    hit = (t < 10) & (nrm != 0).any(dim=1)
    Ld = torch.from_numpy(L.astype(np.float64)).to(og.device)
    nd = nrm.double()
    c = nd[:, 0] * Ld[0] + nd[:, 1] * Ld[1] + nd[:, 2] * Ld[2]
    cast = hit & (c > 0)
    p = spawn(torch, og, dg, t[:, None])
    lit = torch.ones(n, dtype=torch.float32, device=og.device)
    lit[hit & ~cast] = 0
    it2 = torch.zeros(n, dtype=torch.int32, device=og.device)
    sdf2 = torch.zeros(n, dtype=torch.int32, device=og.device)
    so = spawn(torch, p[cast], nrm[cast], BIAS).contiguous()
    sd = torch.from_numpy(L).to(og.device).expand(len(so), 3).contiguous()
    ts, its, cs, _ = ctx.ray_march(so, sd, normal=False)
    lit[cast] = (ts >= 10).float()
    it2[cast] = its
    sdf2[cast] = cs
    ph, nh = p[hit], nrm[hit]
    occ = np.zeros(len(ph), np.float64)
    cnt = np.zeros(len(ph), np.int64)
    for k in range(1, K + 1):
        h = k * AO_STEP
        d, c_k = ctx.scene_distance(spawn(torch, ph, nh, h).cpu().numpy())  # host points only
        occ = occ + (h - d) * 2.0 ** (1 - k)
        cnt += c_k
    x = 1.0 - AO_STRENGTH * occ
    ao = torch.ones(n, dtype=torch.float32, device=og.device)
    ao[hit] = torch.from_numpy(np.where(x > 0, np.where(x > 1, 1.0, x), 0.0).astype(np.float32)).to(og.device)
    sdf2[hit] += torch.from_numpy(cnt.astype(np.int32)).to(og.device)
    return t, it, sdf, nrm, lit, ao, it2, sdf2


def bench(args, torch, R):
    scene, o, d = (rays_c3 if args.case == "C3" else rays_c5)(R)
    ctx = scene.ctx
    L = R.phong_light()
    og, dg = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    out = {}

    def march():
        out["march"] = ctx.ray_march(og, dg, normal=True)

    def light():
        out["light"] = ctx.light(og, dg)
    res = {"case": args.case + " light", "rays": len(o)}
    res["march_ms"] = timed(torch, march, args.warmup, args.reps)
    res["march_kernel"] = ctx.last_kernel()
    res["light_ms"] = timed(torch, light, args.warmup, args.reps)
    res["light_kernel"] = ctx.last_kernel()
    res["light_vs_march"] = res["light_ms"] / res["march_ms"]
    ms = []
    for _ in range(args.composed_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out["composed"] = composed(torch, ctx, og, dg, L)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    res["composed_ms"] = float(np.median(ms))
    res["composed_vs_light"] = res["composed_ms"] / res["light_ms"]
    t, _, _, nrm, lit, ao, it2, sdf2 = (x.cpu().numpy() for x in out["light"])
    hit, cast = classes(t, nrm, L)
    res["hit_fraction"] = float(hit.mean())
    res["cast_fraction"] = float(cast.mean())
    res["shadowed_of_cast"] = float((lit[cast] == 0).mean()) if cast.any() else 0.0
    res["mean_ao_of_hits"] = float(ao[hit].mean()) if hit.any() else 1.0
    res["iters2_per_cast_ray"] = float(it2[cast].mean()) if cast.any() else 0.0
    res["sdf2_per_hit_ray"] = float(sdf2[hit].mean()) if hit.any() else 0.0
    res["hashes"] = {"march": digest(out["march"]), "light_shared": digest(out["light"][:4]), "light": digest(out["light"]),
                     "composed": digest(out["composed"])}
    res["same_hash"] = res["hashes"]["march"] == res["hashes"]["light_shared"] and res["hashes"]["light"] == res["hashes"]["composed"]
    print(json.dumps(res))
    return res["same_hash"]


def counts(args, torch, R):
    W, H, ang = 640, 360, (0.2, 0.5)
    org, dirs = R.camera_rays(W, H, *ang)
    og = torch.from_numpy(np.broadcast_to(org, dirs.shape).copy()).cuda()
    dg = torch.from_numpy(dirs).cuda()
    L = R.phong_light()
    for accel in ("None", "Octree", "BVH"):
        scene = R.Scene(accel)
        scene.loadPreset(3)
        for alg in ALGS:
            t, it, sdf, nrm, lit, ao, it2, sdf2 = (x.cpu().numpy() for x in scene.ctx.light(og, dg, algorithm=alg))
            samples = scene.ctx.light(og, dg, light_dir=(0, 0, 0), algorithm=alg)[7].cpu().numpy()  # no ray is cast: the samples alone
            hit, cast = classes(t, nrm, L)
            nh, nc = max(1, int(hit.sum())), max(1, int(cast.sum()))
            print(json.dumps({"case": "counts", "accel": accel, "algorithm": alg, "rays": len(t), "hits": int(hit.sum()), "cast": int(cast.sum()),
                              "shadowed": int((cast & (lit == 0)).sum()), "primary_iters_per_hit": float(it[hit].sum() / nh),
                              "primary_sdf_per_hit": float(sdf[hit].sum() / nh), "shadow_iters_per_cast": float(it2[cast].sum() / nc),
                              "shadow_sdf_per_cast": float((sdf2[cast].astype(np.int64) - samples[cast]).sum() / nc),
                              "sample_sdf_per_hit": float(samples[hit].sum() / nh), "mean_ao_of_hits": float(ao[hit].mean()) if hit.any() else 1.0}))
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=("C3", "C5", "counts"), required=True)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--composed-reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    if not (counts if args.case == "counts" else bench)(args, torch, R):
        sys.exit(1)


if __name__ == "__main__":
    main()
