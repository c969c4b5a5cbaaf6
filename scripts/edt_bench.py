"""What the exact distance transform of a scene's solid costs (rm_edt_field_device; Context.edt) beside one read of the volume,
beside labelling it and beside the host round trip it replaces.  One GPU, one process.  Run each workload under its own time
limit, e.g.

    timeout -k 10 600 python scripts/edt_bench.py --workload c5 --out profiles/edt/edt_bench.json

Workloads as scripts/parts_bench.py -- `grid` the Dense Grid (125 spheres) under the BVH, `random1000` 1 000 random spheres
under the BVH, `c5` all 10 000 under the octree, the lattice Context.mesh_box's over the scene's box in --cells (256) cells --
and `checkerboard`: no scene, every second point of (cells + 1)^3 in the set: every line's envelope keeps every second
parabola, the deepest stacks there are.  --reps (21) timed repeats after --warmup (2), the figures alternating inside a
repeat; per figure the median, the quartiles and the interquartile range in ms.
  by device events, on a resident float64 volume (the exact field):
    edt_field          rm_edt_field_device alone                  } bytes_per_s: 8 bytes a point over the median
    label_field        rm_label_field_device on the same tensor
    measure_field      rm_measure_field_device on the same tensor: one read of the volume, the floor
  wall clock, to the result on the host:
    edt                Context.edt (the field pass, the transform, one read of the info; d2 stays on the device);
                       checkerboard: Context.edt_field on the resident volume
    scipy_edt          the volume copied to the host and scipy.ndimage.distance_transform_edt there, --scipy-reps (3)
                       repeats; absent, with "scipy": false, where scipy is not importable
sqrt(d2) must equal scipy's distances (where it is importable); the exit status is 1 otherwise.  One JSON line per workload,
merged into --out (a JSON object keyed by workload)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from exact_bench import quartiles, workload  # noqa: E402
from measure_bench import alternate, box_lattice  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=("grid", "random1000", "c5", "checkerboard"), required=True)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--scipy-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    N = R._native
    ctx = R.Context(0)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": args.workload, "reps": args.reps, "cells": args.cells}
    n1 = args.cells + 1
    if args.workload == "checkerboard":
        geom = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (n1,) * 3)
        i = torch.arange(n1, device="cuda")
        vol = torch.where((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0, -1.0, 1.0).to(torch.float64).contiguous()
        end_to_end = lambda: ctx.edt_field(vol, *geom, device=True)  # noqa: E731
    else:
        centers, radii, accel = workload(args.workload)
        ctx.scene_from_spheres(centers, radii, accel)
        res.update(spheres=int(len(radii)), accel="BVH" if accel == 2 else "Octree")
        geom, _, _ = box_lattice(centers, radii, args.cells)
        vol, _ = ctx.field(*geom, count=False, device=True, exact=True)
        end_to_end = lambda: ctx.edt(*geom, device=True)  # noqa: E731
    lat = R.make_lattice(*geom)
    n = vol.numel()
    d2 = torch.empty(n, dtype=torch.int32, device=vol.device)
    labels = torch.empty(n, dtype=torch.int32, device=vol.device)
    info = torch.empty(4, dtype=torch.int64, device=vol.device)
    parts_info = torch.empty(4, dtype=torch.int64, device=vol.device)
    record = torch.empty(22, dtype=torch.int64, device=vol.device)
    L = N.lib()
    entries = {"edt_field": lambda: N.check(ctx._h, L.rm_edt_field_device(ctx._h, C.byref(lat), p(vol), N.RM_MESH_F64, 0.0, 0, p(d2), p(info), stream)),
               "label_field": lambda: N.check(ctx._h, L.rm_label_field_device(ctx._h, C.byref(lat), p(vol), N.RM_MESH_F64, 0.0, 0, p(labels), p(parts_info), stream)),
               "measure_field": lambda: N.check(ctx._h, L.rm_measure_field_device(ctx._h, C.byref(lat), p(vol), N.RM_MESH_F64, 0.0, p(record), stream))}
    ms = alternate(torch, entries, args.warmup, args.reps, True)
    for r in entries:
        res[r] = quartiles(ms[r])
    res["edt_field"]["bytes_per_s"] = round(8 * n / (res["edt_field"]["median_ms"] * 1e-3), 1)
    res["edt_over_label"] = round(res["edt_field"]["median_ms"] / res["label_field"]["median_ms"], 2)
    got = {}
    wall = alternate(torch, {"edt": lambda: got.__setitem__("edt", end_to_end())}, args.warmup, args.reps, False)
    res["edt"] = quartiles(wall["edt"])
    edt = got["edt"]
    head = info.cpu().numpy()
    res.update(points=n, n_set=edt.n_set, max_d2=edt.max_d2, argmax=edt.argmax, step=edt.step)
    ok = torch.equal(edt.d2.reshape(-1), d2) and head.tolist() == [n, edt.n_set, edt.max_d2, edt.argmax]
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    res["scipy"] = ndimage is not None
    if ndimage is not None:
        took = []
        for _ in range(args.scipy_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = vol.cpu().numpy()
            theirs = ndimage.distance_transform_edt(host < 0.0)
            took.append(1e3 * (time.perf_counter() - t0))
        res["scipy_edt"] = quartiles(took)
        ours = edt.d2.cpu().numpy()
        ok = ok and bool((ours < N.RM_EDT_FAR).all()) and np.array_equal(np.sqrt(ours.astype(np.float64)), theirs)
    res["same_results"] = bool(ok)
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
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
