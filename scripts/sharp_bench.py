"""Sharp vertices (rm_scene_sharpen_device: sharp_kernel) on the cells of a mesh that already sits on the device, beside the
attribute pass a host had for a mesh before.  One GPU.  Run under a time limit, e.g.

    timeout -k 10 400 python scripts/sharp_bench.py

Three scenes under the BVH -- the Dense Grid (preset 3), the Pyramid of Boxes (preset 9) and the first 1 000 of the random
spheres of cpu_raymarcher_amd/synthetic.py --, each meshed on 256^3 points over 1.2 times the root box (the volumes of
scripts/mesh_bench.py).  All from one run, the figures alternating inside a repetition:
  (a) sharpen_r0, sharpen_r2   rm_scene_sharpen_device on the resident cell keys with refine = 0 and 2 into preallocated outputs
                               (position, feature, count): HIP-event time of the call, evaluations per vertex from count
  (b) snap3                    rm_scene_points_device on the resident vertices, K = 3 with normals and objects -- the attribute
                               pass of Context.mesh(attributes=True, snap=3) alone: HIP-event time
  (c) mesh_snap3, mesh_sharp   Context.mesh(attributes=True, snap=3, device=True) and Context.mesh(sharp=True, device=True), the
                               whole call from the field to the tensors: wall time ending in a synchronise
Warm-up calls first, then --reps timed ones (21); every figure is the median with the minimum and the maximum beside it.  Also
recorded: how many vertices got which feature, and the mean and largest |getDistance| at the vertices before and after (under a
BVH getDistance over-estimates inside leaf boxes: it is the marchers' bound, not the exact field).  Report only: no comparable
pass existed before this one, so there is no threshold.  The results go to --out (profiles/sharp/sharp_bench.json) and, one JSON
line per scene, to the standard output."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from field_bench import event_ms, wall_ms  # noqa: E402
from mesh_bench import stats  # noqa: E402


def load(R, name):
    scene = R.Scene("BVH")
    if name == "grid":
        scene.loadPreset(3)
    elif name == "pyramid":
        scene.loadPreset(9)
    else:
        from cpu_raymarcher_amd.synthetic import synthetic_spheres
        s = synthetic_spheres(1000)
        scene.loadSpheres(s[:, :3], s[:, 3])
    return scene


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--mesh-reps", type=int, default=5)
    ap.add_argument("--scenes", nargs="+", default=["grid", "pyramid", "spheres1000"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sharp", "sharp_bench.json"))
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    N = R._native
    results = []
    for name in args.scenes:
        scene = load(R, name)
        ctx = scene.ctx
        info = scene.info()
        mn, mx = np.array(info["root_min"]), np.array(info["root_max"])
        c, h = (mn + mx) / 2, 1.2 * (mx - mn) / 2
        shape = (args.size,) * 3
        step = 2 * h / np.array(shape)
        lattice = (c - h + step / 2, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), shape)
        vol, _ = ctx.field(*lattice[:4], shape=shape, count=False, device=True)
        vertices, _ = ctx.mesh_field(vol, *lattice, device=True)
        cells = ctx.mesh_cells(vol, *lattice, device=True)
        del vol
        n = len(vertices)
        res = {"scene": name, "accel": info["accel"], "shape": list(shape), "vertices": n, "prims": info["n_prims"]}
        lat = R.context.make_lattice(*lattice)
        pos = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        feat = torch.empty(n, dtype=torch.int32, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        snapped = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        p_out = [torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda"),
                 torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                 torch.empty(n, dtype=torch.int32, device="cuda")]

        def sharpen(refine):
            q = ctx._sharp_query(0.0, refine, 0.1, 1.0)
            N.check(ctx._h, N.lib().rm_scene_sharpen_device(ctx._h, C.byref(lat), C.byref(q), n, C.c_void_p(cells.data_ptr()), C.c_void_p(pos.data_ptr()),
                                                            C.c_void_p(feat.data_ptr()), C.c_void_p(cnt.data_ptr()), None))

        def snap3():
            q = ctx._point_query(True, 3, 1e-4, 0.0, 0.0)
            N.check(ctx._h, N.lib().rm_scene_points_device(ctx._h, C.byref(q), n, C.c_void_p(vertices.data_ptr()), C.c_void_p(snapped.data_ptr()),
                                                           *[C.c_void_p(b.data_ptr()) for b in p_out], None))

        def residual(points):
            d = ctx.points(points, normal=False, object=False, device=True).dist.abs()
            return {"mean_abs_dist": float(d.mean()), "max_abs_dist": float(d.max())}

        with torch.cuda.stream(torch.cuda.default_stream()):
            runs = {"sharpen_r0": lambda: sharpen(0), "sharpen_r2": lambda: sharpen(2), "snap3": snap3}
            times = {k: [] for k in runs}
            for rep in range(args.warmup + args.reps):
                for k, fn in runs.items():
                    ms = event_ms(torch, fn)
                    if rep >= args.warmup:
                        times[k].append(ms)
            res["surface_nets"] = residual(vertices)
            for refine in (0, 2):
                sharpen(refine)
                kernel = ctx.last_kernel()
                torch.cuda.synchronize()
                counts = cnt.cpu().numpy().view(np.uint32).astype(np.uint64)
                res["sharpen_r%d" % refine] = dict(stats(times["sharpen_r%d" % refine]), counted_per_vertex=round(float(counts.mean()), 2),
                                                   features=np.bincount(feat.cpu().numpy() + 1, minlength=5).tolist(), **residual(pos))
            res["kernel"] = kernel
            snap3()
            res["snap3"] = dict(stats(times["snap3"]), counted_per_vertex=round(float(p_out[4].cpu().numpy().view(np.uint32).astype(np.uint64).mean()), 2),
                                **residual(snapped))
            whole = {"mesh_snap3": lambda: ctx.mesh(*lattice, attributes=True, snap=3, device=True),
                     "mesh_sharp": lambda: ctx.mesh(*lattice, sharp=True, device=True), "mesh_plain": lambda: ctx.mesh(*lattice, device=True)}
            wtimes = {k: [] for k in whole}
            for rep in range(1 + args.mesh_reps):
                for k, fn in whole.items():
                    ms = wall_ms(torch, fn)
                    if rep >= 1:
                        wtimes[k].append(ms)
            for k in whole:
                res[k] = stats(wtimes[k])
        res["sharpen_r2_vs_snap3"] = round(res["sharpen_r2"]["ms"] / res["snap3"]["ms"], 2)
        print(json.dumps(res), flush=True)
        results.append(res)
    doc = {"script": "scripts/sharp_bench.py", "device": "one MI355X",
           "method": "HIP events, %d warm-up calls, median of %d (min - max) for sharpen_r0, sharpen_r2 and snap3, alternating inside a repetition; "
                     "mesh_* are wall times ending in a synchronise, median of %d after one warm-up call; counted_per_vertex is the mean of the count "
                     "output: the primitives evaluated, not the evaluations" % (args.warmup, args.reps, args.mesh_reps),
           "not_measured": ["sharing crossings between the four cells around an edge (not built)", "unordered keys", "refine above 2", "option exact"],
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
