"""Field-query throughput (rm_scene_field_device / rm_scene_field, field_kernel<...>) in points per second, against the
route a host had before: the points formed on the host (rm_lattice_points) and sent through rm_scene_distance.  One GPU.  Run
each step under its own time limit, e.g.

    timeout -k 10 400 python scripts/field_bench.py --scene grid
    timeout -k 10 400 python scripts/field_bench.py --scene spheres

Two workloads -- a 1024 x 1024 slice through the middle of the scene and a 256^3 volume, both 1.2 times the root box -- on
two scenes: the Dense Grid (preset 3) under the BVH and the 10 000 random spheres of cpu_raymarcher_amd/synthetic.py under the
octree.  Three paths, all from the same run:
  (a) device   rm_scene_field_device, dist (f64) and count resident on the device: HIP-event time of the call;
               device32: the same with dist32 alone
  (b) host     rm_scene_field into numpy arrays: wall time, it ends in a synchronise
  (c) points   rm_lattice_points on the host, then rm_scene_distance: wall time (the points alone are reported too)
Warm-up calls first, then --reps timed ones; every figure is the median with the minimum and the maximum beside it.  A build
of the library that carries a second lane mapping behind an option `field_tiles` (how the shipped, linear mapping was chosen:
DESIGN.md 4) has both timed, alternating inside every repetition.  The outputs of all paths must
hash alike; the exit status is 1 otherwise.  One JSON line per workload."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def digest(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).view(np.uint8).tobytes())
    return h.hexdigest()[:16]


def stats(ms, n):
    ms = sorted(ms)
    med = float(np.median(ms))
    return {"ms": round(med, 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "points_per_s": round(n / (med * 1e-3), 1)}


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def load(R, name):
    if name == "grid":
        scene = R.Scene("BVH")
        scene.loadPreset(3)
    else:
        from cpu_raymarcher_amd.synthetic import synthetic_spheres
        s = synthetic_spheres(10000)
        scene = R.Scene("Octree")
        scene.loadSpheres(s[:, :3], s[:, 3])
    return scene


def workloads(info, slice_n, volume_n):
    mn, mx = np.array(info["root_min"]), np.array(info["root_max"])
    c, h = (mn + mx) / 2, 1.2 * (mx - mn) / 2
    for name, shape in (("slice", (slice_n, slice_n, 1)), ("volume", (volume_n, volume_n, volume_n))):
        step = 2 * h / np.array(shape)
        origin = c - h + step / 2
        if shape[2] == 1:
            origin[2] = c[2]
        yield name, origin, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2] if shape[2] > 1 else 0), shape


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", choices=("grid", "spheres"), required=True)
    ap.add_argument("--slice", type=int, default=1024)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    scene = load(R, args.scene)
    ctx = scene.ctx
    mappings = {"linear": 0, "tiled": 1}
    try:
        ctx.set_option("field_tiles", 0)
    except R.RmError:
        mappings = {"shipped": None}  # the library has one lane mapping
    ok = True
    for name, origin, du, dv, dw, shape in workloads(scene.info(), args.slice, args.volume):
        n = shape[0] * shape[1] * shape[2]
        res = {"scene": args.scene, "workload": name, "shape": list(shape), "n": n}
        out, hashes = {}, {}

        def device(key, tiles, dist32):
            def run():
                if tiles is not None:
                    ctx.set_option("field_tiles", tiles)
                out[key] = ctx.field(origin, du, dv, dw, shape=shape, dist32=dist32, count=not dist32, device=True)
            return run
        runs = {}
        for m, tiles in mappings.items():
            runs["device_" + m] = device("device_" + m, tiles, False)
            runs["device32_" + m] = device("device32_" + m, tiles, True)
        times = {k: [] for k in runs}
        for rep in range(args.warmup + args.reps):  # the variants alternate inside a repetition
            for k, fn in runs.items():
                ms = event_ms(torch, fn)
                if rep >= args.warmup:
                    times[k].append(ms)
        for k in runs:
            res[k] = stats(times[k], n)
            hashes[k] = digest(*[x for x in out[k] if x is not None])
        res["kernel"] = ctx.last_kernel()
        for m, tiles in mappings.items():
            def host():
                if tiles is not None:
                    ctx.set_option("field_tiles", tiles)
                out["host"] = ctx.field(origin, du, dv, dw, shape=shape)
            host()
            res["host_" + m] = stats([wall_ms(torch, host) for _ in range(args.host_reps)], n)
            hashes["host_" + m] = digest(*out["host"])
        pts_ms = []

        def points():
            t0 = time.perf_counter()
            p = ctx.lattice_points(origin, du, dv, dw, shape=shape)
            pts_ms.append(1e3 * (time.perf_counter() - t0))
            out["points"] = ctx.scene_distance(p)
        points()
        del pts_ms[:]
        res["points"] = stats([wall_ms(torch, points) for _ in range(args.host_reps)], n)
        res["points_formed_on_host_ms"] = round(float(np.median(pts_ms)), 4)
        hashes["points"] = digest(*out["points"])
        d64 = [v for k, v in hashes.items() if not k.startswith("device32")]
        d32 = [v for k, v in hashes.items() if k.startswith("device32")]
        want32 = digest(out["points"][0].astype(np.float32))
        res["same_hash"] = len(set(d64)) == 1 and set(d32) == {want32}
        res["hash"] = d64[0]
        first = "linear" if "linear" in mappings else "shipped"
        res["device_vs_points"] = round(res["points"]["ms"] / res["device_" + first]["ms"], 2)
        res["host_vs_points"] = round(res["points"]["ms"] / res["host_" + first]["ms"], 2)
        if "tiled" in mappings:
            res["tiled_vs_linear"] = round(res["device_tiled"]["ms"] / res["device_linear"]["ms"], 4)
            res["tiled32_vs_linear32"] = round(res["device32_tiled"]["ms"] / res["device32_linear"]["ms"], 4)
        d = out["points"][0]
        res["inside_fraction"] = round(float((d < 0).mean()), 4)
        res["mean_count"] = round(float(out["points"][1].mean()), 2)
        print(json.dumps(res), flush=True)
        ok = ok and res["same_hash"]
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
