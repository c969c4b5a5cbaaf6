"""What measuring a scene costs (rm_measure_field_device, rm_measure_tiles_device; Context.measure, MeshSession.measure) beside
the work it rides on.  One GPU, one process.  Run each workload under its own time limit, e.g.

    timeout -k 10 600 python scripts/measure_bench.py --workload c5 --out profiles/measure/measure_bench.json

Workloads as scripts/exact_bench.py: `grid` the Dense Grid (125 spheres) under the BVH, `random1000` 1 000 random spheres under
the BVH, `c5` all 10 000 under the octree; the lattice is Context.mesh_box's over the scene's box in --cells (256) cells, and in
--sparse-cells (1024) cells for the sparse figures alone.  --reps (21) timed repeats after --warmup (2), the figures of a group
alternating inside a repeat; per figure the median, the quartiles and the interquartile range in ms.
  dense (by device events, on a resident float64 volume of the exact field):
    measure_field      rm_measure_field_device alone                       } bytes_per_s: 8 bytes a point over the median
    torch_count        (values < iso).sum() in torch on the same tensor    } -- the yardstick for one pass over the data
  sparse, per lattice:
    measure            Context.measure(sparse=True), wall clock to the record on the host
    mesh_sparse        Context.mesh_sparse(exact=True, order="tile", device=True), wall clock, a synchronisation last
    measure_tiles      rm_measure_tiles_device alone, by events             } over the same resident tiles
    mesh_count         rm_mesh_tiles_device's counting call alone, by events }
  session (--cells lattice; per repeat one random sphere moves by a tenth of the box, as scripts/remesh_bench.py):
    edit_measure       MeshSession.edit_spheres + MeshSession.measure(), wall clock
    edit_mesh          MeshSession.edit_spheres + MeshSession.mesh(order="tile", device=True), wall clock
The sparse record must equal the dense one (the block fields and n_nonfinite apart) and the session's record the one measured
from scratch; the exit status is 1 otherwise.  One JSON line per workload, merged into --out (a JSON object keyed by workload)."""
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

APART = ("n_blocks", "n_kept", "n_blocks_inside", "n_nonfinite")


def same(a, b):
    return all(x == y for f, x, y in zip(a._fields, a, b) if f not in APART)


def box_lattice(centers, radii, n):
    c64 = centers.astype(np.float64)
    lo, hi = (c64 - radii[:, None]).min(axis=0), (c64 + radii[:, None]).max(axis=0)
    m = 2 * (hi - lo) / (n - 4)  # Context.mesh_box's margin for iso 0
    step = (hi - lo + 2 * m) / n
    return (lo - m, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), (n + 1,) * 3), lo, hi


def alternate(torch, runs, warmup, reps, events):
    """name -> list of ms; the order of the runs turns round every repeat."""
    ms = {r: [] for r in runs}
    names = tuple(runs)
    for rep in range(warmup + reps):
        for r in names[rep % len(names):] + names[:rep % len(names)]:
            if events:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                runs[r]()
                b.record()
                torch.cuda.synchronize()
                t = a.elapsed_time(b)
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs[r]()
                torch.cuda.synchronize()
                t = 1e3 * (time.perf_counter() - t0)
            if rep >= warmup:
                ms[r].append(t)
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=("grid", "random1000", "c5"), required=True)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--sparse-cells", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    N = R._native
    centers, radii, accel = workload(args.workload)
    ctx = R.Context(0)
    ctx.scene_from_spheres(centers, radii, accel)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": args.workload, "spheres": int(len(radii)), "accel": "BVH" if accel == 2 else "Octree", "reps": args.reps}
    ok = True

    # ---- the dense entry beside torch's count, on one resident volume
    geom, lo, hi = box_lattice(centers, radii, args.cells)
    lat = R.make_lattice(*geom)
    vol, _ = ctx.field(*geom, count=False, device=True, exact=True)
    n = vol.numel()
    record = torch.empty(22, dtype=torch.int64, device=vol.device)
    counted = []
    dense_runs = {"measure_field": lambda: N.check(ctx._h, N.lib().rm_measure_field_device(ctx._h, C.byref(lat), p(vol), N.RM_MESH_F64, 0.0, p(record), stream)),
                  "torch_count": lambda: counted.append((vol < 0.0).sum())}
    ms = alternate(torch, dense_runs, args.warmup, args.reps, True)
    dense = ctx.measure_field(vol, *geom)
    ok = ok and dense.n_inside == int(counted[-1])
    res["dense"] = {"cells": args.cells, "points": n, "n_inside": dense.n_inside, "volume": dense.world.volume, "area_estimate": dense.world.area_estimate}
    for r in dense_runs:
        res["dense"][r] = quartiles(ms[r])
        res["dense"][r]["bytes_per_s"] = round(8 * n / (res["dense"][r]["median_ms"] * 1e-3), 1)
    del vol, counted

    # ---- the sparse path, end to end and its last entry alone, beside the sparse mesher on the same lattice
    res["sparse"] = {}
    for cells in (args.cells, args.sparse_cells):
        geom, _, _ = box_lattice(centers, radii, cells)
        lat = R.make_lattice(*geom)
        got = {}
        wall = alternate(torch, {"measure": lambda: got.__setitem__("measure", ctx.measure(*geom)),
                                 "mesh_sparse": lambda: got.__setitem__("mesh", ctx.mesh_sparse(*geom, exact=True, order="tile", device=True))},
                         args.warmup, args.reps, False)
        blocks = ctx.sparse_blocks(*geom, dist=True)
        k = blocks.n_kept
        tiles = torch.empty((max(k, 1), 729), dtype=torch.float64, device=blocks.slot.device)
        with ctx._exact(True):
            ctx._tiles_into(lat, blocks.list, k, tiles)
        info = torch.zeros(4, dtype=torch.int64, device=tiles.device)
        lst = blocks.list.contiguous()
        entries = {"measure_tiles": lambda: N.check(ctx._h, N.lib().rm_measure_tiles_device(ctx._h, C.byref(lat), p(blocks.slot), p(lst), k, p(blocks.dist), p(tiles),
                                                                                            0.0, p(record), stream)),
                   "mesh_count": lambda: N.check(ctx._h, N.lib().rm_mesh_tiles_device(ctx._h, C.byref(lat), p(blocks.slot), p(lst), k, p(tiles), 0.0, None, 0, None, 0,
                                                                                      None, None, p(info), stream))}
        ev = alternate(torch, entries, args.warmup, args.reps, True)
        m = got["measure"]
        if cells == args.cells:
            ok = ok and same(m, dense)
        ok = ok and m == ctx._measure_tiles(lat, blocks.slot, lst, k, blocks.dist, tiles, 0.0)
        out = {"points": (cells + 1) ** 3, "n_blocks": m.n_blocks, "n_kept": m.n_kept, "n_blocks_inside": m.n_blocks_inside, "n_inside": m.n_inside,
               "volume": m.world.volume, "vertices": int(len(got["mesh"][0])), "tile_bytes": 8 * 729 * k}
        for r in wall:
            out[r] = quartiles(wall[r])
        for r in ev:
            out[r] = quartiles(ev[r])
        out["measure_tiles"]["bytes_per_s"] = round(8 * 729 * k / (out["measure_tiles"]["median_ms"] * 1e-3), 1)
        res["sparse"][str(cells)] = out
        del got, tiles, blocks

    # ---- after a one-sphere edit: the session's measure beside its mesh
    geom, lo, hi = box_lattice(centers, radii, args.cells)
    session = ctx.mesh_session(*geom)
    rng = np.random.default_rng(args.seed)
    cur = centers.copy()

    def edit():
        i = int(rng.integers(0, len(radii)))
        d = rng.normal(size=3)
        cur[i] = (cur[i].astype(np.float64) + 0.1 * float((hi - lo).max()) * d / np.linalg.norm(d)).astype(np.float32)
        session.edit_spheres([("set", i, cur[i], float(radii[i]))])

    shares = []
    routes = {"edit_measure": lambda: (edit(), session.measure(), shares.append(session.stats["n_reused"] / max(1, session.stats["n_kept"]))),
              "edit_mesh": lambda: (edit(), session.mesh(order="tile", device=True))}
    ms = alternate(torch, routes, args.warmup, args.reps, False)
    ok = ok and session.measure() == ctx.measure(*geom)
    res["session"] = {"cells": args.cells, "reused_share_median": round(float(np.median(shares)), 4)}
    for r in routes:
        res["session"][r] = quartiles(ms[r])
    res["same_records"] = bool(ok)
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
