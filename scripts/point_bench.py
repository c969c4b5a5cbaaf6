"""Point queries (rm_scene_points_device: point_kernel) on the vertices of a mesh that already sit on the device, against the
route a host had before for normals alone.  One GPU.  Run under a time limit, e.g.

    timeout -k 10 300 python scripts/point_bench.py

Two vertex sets -- the 256^3 surface-nets mesh of the Dense Grid (preset 3) under the BVH and of the 10 000 random spheres of
cpu_raymarcher_amd/synthetic.py under the octree, over 1.2 times the root box (the volumes of scripts/mesh_bench.py) --, each
with K = 0 and K = 3 projection steps, normals and objects on.  All from one run:
  (a) points    rm_scene_points_device on the resident vertices into preallocated outputs (all six): HIP-event time of the call
  (b) host      the route without the entry, normals alone: download the vertices, four rm_scene_distance calls (the point and
                its three offsets by -0.01) and getNormal's arithmetic in numpy; wall time.  It has no object and no projection.
Warm-up calls first, then --reps timed ones; every figure is the median with the minimum and the maximum beside it.  The
normals of (a) with K = 0 and of (b) must be the same bytes; the exit status is 1 otherwise.  Also recorded: the largest
|dist - iso| over the vertices before (K = 0) and after the snap, and how many steps the vertices took.  The results go to
--out (profiles/points/point_bench.json) and, one JSON line per workload, to the standard output."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from field_bench import event_ms, load, wall_ms  # noqa: E402
from mesh_bench import stats  # noqa: E402


def host_normals(ctx, d_vertices):
    """What a host did for normals without the entry: the vertices come down, Scene.getDistance four times, numpy."""
    p = d_vertices.cpu().numpy()
    d0, _ = ctx.scene_distance(p)
    n = np.zeros_like(p)
    for c in range(3):
        q = p.copy()
        q[:, c] = (p[:, c].astype(np.float64) - 0.01).astype(np.float32)
        n[:, c] = (d0 - ctx.scene_distance(q)[0]).astype(np.float32)
    w = n.astype(np.float64)
    length = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
    with np.errstate(all="ignore"):
        scale = np.where(length > 0, 1 / np.sqrt(np.where(length > 0, length, 1.0)), length)
    return (w * scale[:, None]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "points", "point_bench.json"))
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    N = R._native
    results, ok = [], True
    for name in ("grid", "spheres"):
        scene = load(R, name)
        ctx = scene.ctx
        info = scene.info()
        mn, mx = np.array(info["root_min"]), np.array(info["root_max"])
        c, h = (mn + mx) / 2, 1.2 * (mx - mn) / 2
        shape = (args.size,) * 3
        step = 2 * h / np.array(shape)
        vertices, _ = ctx.mesh(c - h + step / 2, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), shape, device=True)
        n = len(vertices)
        res = {"scene": name, "accel": info["accel"], "shape": list(shape), "vertices": n}
        out = [torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"),
               torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
               torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")]

        def entry(k):
            q = ctx._point_query(True, k, 1e-4, 0.0, 0.0)
            N.check(ctx._h, N.lib().rm_scene_points_device(ctx._h, C.byref(q), n, C.c_void_p(vertices.data_ptr()),
                                                           *[C.c_void_p(b.data_ptr()) for b in out], None))
        with torch.cuda.stream(torch.cuda.default_stream()):
            times = {0: [], 3: []}
            for rep in range(args.warmup + args.reps):  # the two figures alternate inside a repetition
                for k in times:
                    ms = event_ms(torch, lambda: entry(k))
                    if rep >= args.warmup:
                        times[k].append(ms)
            for k in times:
                entry(k)
                torch.cuda.synchronize()
                dist, steps = out[1].cpu().numpy(), out[4].cpu().numpy()
                res["points_k%d" % k] = dict(stats(times[k]), max_abs_dist=float(np.abs(dist).max()), steps=np.bincount(steps, minlength=k + 1).tolist(),
                                             sdf_calls=int(out[5].cpu().numpy().view(np.uint32).astype(np.uint64).sum()))
                if k == 0:
                    normals = out[2].cpu().numpy()
                    res["objects"] = int(len(np.unique(out[3].cpu().numpy())))
        res["kernel"] = ctx.last_kernel()
        got = {}

        def host():
            got["n"] = host_normals(ctx, vertices)
        host()
        res["host_normals"] = stats([wall_ms(torch, host) for _ in range(args.host_reps)])
        res["same_normals"] = got["n"].tobytes() == normals.tobytes()
        res["host_vs_points_k0"] = round(res["host_normals"]["ms"] / res["points_k0"]["ms"], 2)
        print(json.dumps(res), flush=True)
        results.append(res)
        ok = ok and res["same_normals"]
    doc = {"script": "scripts/point_bench.py", "device": "one MI355X",
           "method": "HIP events, %d warm-up calls, median of %d (min - max); host_normals is a wall time ending in a synchronise, median of %d"
                     % (args.warmup, args.reps, args.host_reps),
           "not_measured": ["wave compaction of converged lanes (not built)", "point sets without spatial order", "per-output cost"],
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
