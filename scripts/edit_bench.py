"""What one interactive edit costs: move one sphere, render 256 x 256, synchronise -- by three routes, in one process.  One GPU.
Run each workload under its own time limit, e.g.

    timeout -k 10 300 python scripts/edit_bench.py --workload grid --out profiles/edit/edit_bench.json

Workloads: `grid` the Dense Grid (preset 3, 125 spheres) under the BVH, `random1000` 1 000 of the random spheres of
cpu_raymarcher_amd/synthetic.py under the BVH, `c5` all 10 000 of them under the octree.  Routes:
  (a) upload    rm_scene_from_spheres with the moved list: what a host had before rm_scene_edit_spheres
  (b) edit_host rm_scene_edit_spheres with option device_build = 0 (the host builder for everything)
  (c) edit_dev  rm_scene_edit_spheres with device_build = 1 (the four pair loops on the device: csrc/rm_scene_build.hip)
Every repeat moves one sphere by a different small offset, renders once and waits for the stream; the three routes alternate
inside a repeat and see the same offsets.  --reps (21) timed repeats after --warmup (2); per route the median, the quartiles
and the interquartile range of the wall time in ms, and the split between the scene update and the render.  The frames of the
three routes must hash alike in every repeat; the exit status is 1 otherwise.  One JSON line per workload, merged into --out
(a JSON object keyed by workload) when that is given."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BVH, OCTREE = 2, 1


def workload(name):
    from cpu_raymarcher_amd.synthetic import synthetic_spheres
    if name == "grid":
        c = np.array([(x * 0.6 - 1.2, y * 0.6 - 1.2, z * 0.6 - 1.2) for x in range(5) for y in range(5) for z in range(5)])
        return c.astype(np.float32), np.full(125, 0.15), BVH, 62
    s = synthetic_spheres(1000 if name == "random1000" else 10000)
    return np.ascontiguousarray(s[:, :3], np.float32), np.ascontiguousarray(s[:, 3], np.float64), (BVH if name == "random1000" else OCTREE), 123


def quartiles(ms):
    q1, med, q3 = (float(v) for v in np.percentile(ms, [25, 50, 75]))
    return {"median_ms": round(med, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "iqr_ms": round(q3 - q1, 3),
            "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=("grid", "random1000", "c5"), required=True)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    from cpu_raymarcher_amd import _native as N
    centers, radii, accel, which = workload(args.workload)
    W = H = args.size
    dev = torch.device("cuda", 0)
    bufs = (torch.empty(W * H, dtype=torch.uint8, device=dev), torch.empty(3 * W * H, dtype=torch.uint8, device=dev),
            torch.empty(W * H, dtype=torch.int16, device=dev), torch.empty(W * H, dtype=torch.int16, device=dev))
    job = N.rm_job()
    job.width = job.height = job.y_end = W
    job.camera_pitch, job.camera_yaw = 0.2, 0.5
    job.algorithm = N.lib().rm_algorithm_from_string(b"sphere-tracer")
    job.scene_preset_index = N.RM_SCENE_UPLOADED
    job.acceleration_structure = accel
    job.overshoot_factor = job.step_size = float("nan")
    routes = ("upload", "edit_host", "edit_dev")
    ctxs = {r: R.Context(0) for r in routes}
    for r, ctx in ctxs.items():
        ctx.scene_from_spheres(centers, radii, accel)
        ctx.set_option("device_build", 1 if r == "edit_dev" else 0)
    total = {r: [] for r in routes}
    update = {r: [] for r in routes}
    same = True
    rng = np.random.default_rng(1)
    for rep in range(args.warmup + args.reps):
        moved = centers.copy()
        moved[which] = (centers[which].astype(np.float64) + rng.uniform(-0.05, 0.05, 3)).astype(np.float32)
        hashes = []
        for r in routes:
            ctx = ctxs[r]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if r == "upload":
                ctx.scene_from_spheres(moved, radii, accel)
            else:
                ctx.edit_spheres([("set", which, moved[which], radii[which])])
            t1 = time.perf_counter()
            ctx.render_tile(job, *bufs)
            torch.cuda.current_stream().synchronize()
            t2 = time.perf_counter()
            if rep >= args.warmup:
                total[r].append(1e3 * (t2 - t0))
                update[r].append(1e3 * (t1 - t0))
            h = hashlib.sha256()
            for b in bufs:
                h.update(b.cpu().numpy().tobytes())
            hashes.append(h.hexdigest()[:16])
        same = same and len(set(hashes)) == 1
    res = {"workload": args.workload, "spheres": int(len(radii)), "accel": "BVH" if accel == BVH else "Octree", "frame": [W, H],
           "reps": args.reps, "same_frames": same, "kernel": ctxs["edit_dev"].last_kernel()}
    for r in routes:
        res[r] = quartiles(total[r])
        res[r]["scene_update_median_ms"] = round(float(np.median(update[r])), 3)
    a, c = res["upload"], res["edit_dev"]
    res["dev_vs_upload"] = round(a["median_ms"] / c["median_ms"], 2)
    res["dev_below_upload_by_more_than_the_larger_iqr"] = bool(a["median_ms"] - c["median_ms"] > max(a["iqr_ms"], c["iqr_ms"]))
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                merged = json.load(f)
        merged[args.workload] = res
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)
            f.write("\n")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
