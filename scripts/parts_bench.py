"""What labelling the connected parts of a scene costs (rm_label_field_device, rm_measure_labels_device; Context.parts) beside
one read of the volume and beside the host round trip it replaces.  One GPU, one process.  Run each workload under its own time
limit, e.g.

    timeout -k 10 600 python scripts/parts_bench.py --workload c5 --out profiles/parts/parts_bench.json

Workloads as scripts/exact_bench.py -- `grid` the Dense Grid (125 spheres) under the BVH, `random1000` 1 000 random spheres
under the BVH, `c5` all 10 000 under the octree, the lattice Context.mesh_box's over the scene's box in --cells (256) cells --
`sphere`: preset 0, one sphere of radius 1.5 in [-2, 2]^3 -- one part that holds a fifth of the lattice, so every wave of the
records' pass adds into ONE record: the worst case for its atomics --, and `checkerboard`: no scene, every second point of (cells + 1)^3 in the set, each a part of its own: the worst case for the
numbering (of its 8.5 M parts the first --records get a record).  --reps (21) timed repeats after --warmup (2), the figures
alternating inside a repeat; per figure the median, the quartiles and the interquartile range in ms.
  by device events, on a resident float64 volume (the exact field):
    label_field        rm_label_field_device alone        } bytes_per_s: 8 bytes a point over the median
    measure_labels     rm_measure_labels_device alone, --records (64) records
    measure_field      rm_measure_field_device on the same tensor: one read of the volume, the floor
  wall clock, to the result on the host:
    parts              Context.parts (the field pass, the labels, the records, one read; the labels stay on the device);
                       checkerboard: Context.label_field on the resident volume
    scipy_label        the volume copied to the host and scipy.ndimage.label there, --scipy-reps (3) repeats; absent, with
                       "scipy": false, where scipy is not importable
The labels must equal scipy's (where it is importable) and the records must add up to rm_measure_field_device's record; the
exit status is 1 otherwise.  One JSON line per workload, merged into --out (a JSON object keyed by workload)."""
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

SHARED = ("n_inside", "sum1", "sum2", "crossings")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=("grid", "random1000", "c5", "sphere", "checkerboard"), required=True)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--scipy-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    N = R._native
    ctx = R.Context(0)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": args.workload, "reps": args.reps, "cells": args.cells, "records": args.records}
    n1 = args.cells + 1
    if args.workload == "checkerboard":
        geom = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (n1,) * 3)
        i = torch.arange(n1, device="cuda")
        vol = torch.where((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0, -1.0, 1.0).to(torch.float64).contiguous()
        end_to_end = lambda: ctx.label_field(vol, *geom, records=args.records, device=True)  # noqa: E731
    elif args.workload == "sphere":
        ctx.scene_from_preset(0, 2)
        res.update(spheres=1, accel="BVH")
        geom = ((-2.0,) * 3, (4.0 / args.cells, 0, 0), (0, 4.0 / args.cells, 0), (0, 0, 4.0 / args.cells), (n1,) * 3)
        vol, _ = ctx.field(*geom, count=False, device=True, exact=True)
        end_to_end = lambda: ctx.parts(*geom, records=args.records, device=True)  # noqa: E731
    else:
        centers, radii, accel = workload(args.workload)
        ctx.scene_from_spheres(centers, radii, accel)
        res.update(spheres=int(len(radii)), accel="BVH" if accel == 2 else "Octree")
        geom, _, _ = box_lattice(centers, radii, args.cells)
        vol, _ = ctx.field(*geom, count=False, device=True, exact=True)
        end_to_end = lambda: ctx.parts(*geom, records=args.records, device=True)  # noqa: E731
    lat = R.make_lattice(*geom)
    n = vol.numel()
    labels = torch.empty(n, dtype=torch.int32, device=vol.device)
    info = torch.empty(4, dtype=torch.int64, device=vol.device)
    records = torch.empty(22 * max(args.records, 1), dtype=torch.int64, device=vol.device)
    record = torch.empty(22, dtype=torch.int64, device=vol.device)
    L = N.lib()
    entries = {"label_field": lambda: N.check(ctx._h, L.rm_label_field_device(ctx._h, C.byref(lat), p(vol), N.RM_MESH_F64, 0.0, 0, p(labels), p(info), stream)),
               "measure_labels": lambda: N.check(ctx._h, L.rm_measure_labels_device(ctx._h, C.byref(lat), p(labels), args.records, p(records), stream)),
               "measure_field": lambda: N.check(ctx._h, L.rm_measure_field_device(ctx._h, C.byref(lat), p(vol), N.RM_MESH_F64, 0.0, p(record), stream))}
    entries["label_field"]()  # the labels the second entry reads
    ms = alternate(torch, entries, args.warmup, args.reps, True)
    for r in entries:
        res[r] = quartiles(ms[r])
    res["label_field"]["bytes_per_s"] = round(8 * n / (res["label_field"]["median_ms"] * 1e-3), 1)
    got = {}
    wall = alternate(torch, {"parts": lambda: got.__setitem__("parts", end_to_end())}, args.warmup, args.reps, False)
    res["parts"] = quartiles(wall["parts"])
    parts = got["parts"]
    res.update(points=n, n_set=parts.n_set, n_parts=parts.n_parts, gave_up=int(info.cpu()[3]),
               largest=[parts.measures[q].n_inside for q in parts.by_size()[:4]])
    ok = res["gave_up"] == 0 and torch.equal(parts.labels.reshape(-1), labels)
    # the records of all parts add up to the measure of the whole
    if parts.n_parts <= (1 << 20):
        every = ctx.label_field(vol, *geom, records=parts.n_parts, device=True)
        whole = ctx.measure_field(vol, *geom)
        for f in SHARED:
            total = np.sum([np.asarray(getattr(m, f), dtype=object) for m in every.measures], axis=0)
            ok = ok and len(every.measures) == every.n_parts and bool((np.asarray(total) == np.asarray(getattr(whole, f), dtype=object)).all())
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
            theirs, count = ndimage.label(host < 0.0)
            took.append(1e3 * (time.perf_counter() - t0))
        res["scipy_label"] = quartiles(took)
        ok = ok and count == parts.n_parts and np.array_equal(theirs.astype(np.int32) - 1, parts.labels.cpu().numpy())
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
