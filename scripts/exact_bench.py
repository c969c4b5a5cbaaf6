"""What option `exact` costs and buys: point queries and sparse meshes from the exact field against the same calls on the
scene's own field and on a second context that holds the scene under acceleration None -- the only way to the exact answers
without the option.  One GPU.  Run each workload under its own time limit, e.g.

    timeout -k 10 600 python scripts/exact_bench.py --workload c5 --out profiles/exact/exact_bench.json

Workloads: `grid` the Dense Grid (preset 3, 125 spheres) under the BVH, `random1000` 1 000 of the random spheres of
cpu_raymarcher_amd/synthetic.py under the BVH, `c5` all 10 000 of them under the octree.  Per workload, in one process:
  (a) points        Context.points with normals, objects and three snap steps on the vertices of the scene's 256^3 mesh
  (b) points_exact  the same with exact=True
  (c) points_none   the same on the acceleration-None context
  (d) mesh, mesh_exact, mesh_none   mesh_sparse over 256^3 cells, likewise
  (e) residual      |dist - iso| after the snap, for (a) and (b): median, 99th percentile, maximum
The vertices are on the device, so are the results; a timed call ends with a synchronisation.  --reps (21) timed repeats after
--warmup (2), the routes alternating inside a repeat; per route the median, the quartiles and the interquartile range in ms.
(b) and (c) must return the same bytes, and so must the two exact meshes; the exit status is 1 otherwise.  One JSON line per
workload, merged into --out (a JSON object keyed by workload) when that is given."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NONE, OCTREE, BVH = 0, 1, 2


def workload(name):
    from cpu_raymarcher_amd.synthetic import synthetic_spheres
    if name == "grid":
        c = np.array([(x * 0.6 - 1.2, y * 0.6 - 1.2, z * 0.6 - 1.2) for x in range(5) for y in range(5) for z in range(5)])
        return c.astype(np.float32), np.full(125, 0.15), BVH
    s = synthetic_spheres(1000 if name == "random1000" else 10000)
    return np.ascontiguousarray(s[:, :3], np.float32), np.ascontiguousarray(s[:, 3], np.float64), (BVH if name == "random1000" else OCTREE)


def quartiles(ms):
    q1, med, q3 = (float(v) for v in np.percentile(ms, [25, 50, 75]))
    return {"median_ms": round(med, 3), "q1_ms": round(q1, 3), "q3_ms": round(q3, 3), "iqr_ms": round(q3 - q1, 3),
            "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=("grid", "random1000", "c5"), required=True)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--iso", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    centers, radii, accel = workload(args.workload)
    ctx, none = R.Context(0), R.Context(0)
    ctx.scene_from_spheres(centers, radii, accel)
    none.scene_from_spheres(centers, radii, NONE)
    c64 = centers.astype(np.float64)
    box = ((c64 - radii[:, None]).min(axis=0), (c64 + radii[:, None]).max(axis=0))
    cells = (args.cells,) * 3

    def mesh(c, exact):
        return c.mesh_box(cells, iso=args.iso, device=True, box=box, sparse=True, exact=exact)

    vertices = mesh(ctx, True)[0].contiguous()

    def points(c, exact):
        return c.points(vertices, normal=True, object=True, snap=3, iso=args.iso, exact=exact)

    routes = {"points": lambda: points(ctx, False), "points_exact": lambda: points(ctx, True), "points_none": lambda: points(none, False),
              "mesh": lambda: mesh(ctx, False), "mesh_exact": lambda: mesh(ctx, True), "mesh_none": lambda: mesh(none, False)}
    ms = {r: [] for r in routes}
    last = {}
    for rep in range(args.warmup + args.reps):
        for r, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[r] = call()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ms[r].append(1e3 * (time.perf_counter() - t0))

    def same(a, b):
        return all((x is None and y is None) or (x.shape == y.shape and bool((x.view(torch.uint8) == y.view(torch.uint8)).all())) for x, y in zip(a, b))

    e, n = last["points_exact"], last["points_none"]
    same_points = same((e.position, e.dist, e.normal, e.object, e.steps), (n.position, n.dist, n.normal, n.object, n.steps))
    same_mesh = same(last["mesh_exact"], last["mesh_none"])
    res = {"workload": args.workload, "spheres": int(len(radii)), "accel": "BVH" if accel == BVH else "Octree", "cells": args.cells, "iso": args.iso,
           "reps": args.reps, "vertices": int(len(vertices)), "exact_tree": ctx.exact_tree(), "exact_points_equal_none": same_points,
           "exact_mesh_equals_none": same_mesh, "mesh_vertices": {r: int(len(last[r][0])) for r in ("mesh", "mesh_exact", "mesh_none")}}
    for r in routes:
        res[r] = quartiles(ms[r])
    for r in ("points", "points_exact"):
        resid = (last[r].dist - args.iso).abs().cpu().numpy()
        res[r]["residual"] = {"median": float(np.median(resid)), "p99": float(np.percentile(resid, 99)), "max": float(resid.max())}
        res[r]["mean_count"] = round(float((last[r].count.cpu().numpy().view(np.uint32)).mean()), 2)
    b, c = res["points_exact"], res["points_none"]
    res["exact_vs_none_points"] = round(c["median_ms"] / b["median_ms"], 2)
    res["exact_points_below_none_by_more_than_the_larger_iqr"] = bool(c["median_ms"] - b["median_ms"] > max(b["iqr_ms"], c["iqr_ms"]))
    res["exact_vs_none_mesh"] = round(res["mesh_none"]["median_ms"] / res["mesh_exact"]["median_ms"], 2)
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
    if not (same_points and same_mesh):
        sys.exit(1)


if __name__ == "__main__":
    main()
