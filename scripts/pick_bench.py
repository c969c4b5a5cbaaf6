"""Object-pick throughput (rm_ray_pick_device, pick_kernel<...>) against ray queries with normals (rm_ray_march_device,
cast_kernel<...>) on the same rays, one GPU.  Run each step under its own time limit, e.g.

    timeout -k 10 300 python scripts/pick_bench.py --case C3
    timeout -k 10 300 python scripts/pick_bench.py --case C5

C3: the 3840 x 2160 camera rays of the Dense Sphere Grid (BVH, angles 0.2 / 0.5) in 8 x 8-tile order (the wave tiles of the
one-ray-per-lane render).  C5: 1 M random rays from inside the octree cube through the 10 000-sphere scene, the
rays of scripts/ray_bench.py.  Times are HIP-event kernel times (median of --reps launches after --warmup).  The outputs the
two entries share (t, iters, sdf_calls, normal) must hash alike; the exit status is 1 otherwise.  One JSON line per case."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ray_bench import timed  # noqa: E402


def shared_hash(out):
    h = hashlib.sha256()
    for x in out[:4]:
        h.update(np.ascontiguousarray(x.cpu().numpy()).tobytes())
    return h.hexdigest()[:16]


def rays_c3(R):
    W, H, ang = 3840, 2160, (0.2, 0.5)
    scene = R.Scene("BVH")
    scene.loadPreset(3)
    org, dirs = R.camera_rays(W, H, *ang)
    y, x = np.divmod(np.arange(W * H), W)
    d = dirs[np.lexsort((x % 8, y % 8, x // 8, y // 8))]
    return scene, np.broadcast_to(org, d.shape).copy(), np.ascontiguousarray(d)


def rays_c5(R):
    from cpu_raymarcher_amd.synthetic import synthetic_spheres
    scene = R.Scene("Octree")
    sp = synthetic_spheres(10000)
    scene.loadSpheres(sp[:, :3], sp[:, 3])
    n = 1 << 20
    vals = np.empty(6 * n, np.uint64)
    with np.errstate(over="ignore"):  # splitmix64, as scripts/ray_bench.py
        k = np.arange(1, 6 * n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x5EED)
        z = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        vals[:] = z ^ (z >> np.uint64(31))
    u = (vals >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    o = (u[:3 * n].reshape(n, 3) * 19.5 - 9.75).astype(np.float32)
    d = (u[3 * n:].reshape(n, 3) * 2 - 1).astype(np.float32)
    return scene, o, d


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=("C3", "C5"), required=True)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    scene, o, d = (rays_c3 if args.case == "C3" else rays_c5)(R)
    ctx = scene.ctx
    og, dg = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    out = {}

    def march():
        out["march"] = ctx.ray_march(og, dg, normal=True)

    def pick():
        out["pick"] = ctx.pick(og, dg, normal=True)
    res = {"case": args.case + " pick", "rays": len(o)}
    res["march_ms"] = timed(torch, march, args.warmup, args.reps)
    res["march_kernel"] = ctx.last_kernel()
    res["pick_ms"] = timed(torch, pick, args.warmup, args.reps)
    res["pick_kernel"] = ctx.last_kernel()
    res["pick_vs_march"] = res["pick_ms"] / res["march_ms"]
    obj = out["pick"][4].cpu().numpy()
    res["hit_fraction"] = float((obj >= 0).mean())
    res["hashes"] = {"march": shared_hash(out["march"]), "pick": shared_hash(out["pick"])}
    res["same_hash"] = res["hashes"]["march"] == res["hashes"]["pick"]
    print(json.dumps(res))
    if not res["same_hash"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
