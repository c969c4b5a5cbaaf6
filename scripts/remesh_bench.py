"""What a mesh session buys in the loop pick -> edit -> look again: re-meshing a sphere scene after a one-sphere edit from the
tiles the edit cannot reach (Context.mesh_session, rm_scene_tiles_update_device) against the full exact sparse path, the only
route there was.  One GPU.  Run each workload under its own time limit, e.g.

    timeout -k 10 600 python scripts/remesh_bench.py --workload c5 --out profiles/remesh/remesh_bench.json

Workloads as scripts/exact_bench.py: `grid` the Dense Grid (125 spheres) under the BVH, `random1000` 1 000 random spheres under
the BVH, `c5` all 10 000 under the octree; the lattice is Context.mesh_box's over the scene's box in --cells (256) cells.  Two
contexts hold the same scene; per repeat one random sphere moves by a tenth of the box in a random direction, in both:
  (a) full     Context.edit_spheres + Context.mesh_sparse(exact=True, order="tile")
  (b) session  MeshSession.edit_spheres + MeshSession.mesh(order="tile")
The meshes stay on the device; a timed route ends with a synchronisation.  --reps (21) timed repeats after --warmup (2), the
two routes alternating inside a repeat (the first to run changes every repeat); per route the median, the quartiles and the
interquartile range in ms.  Both routes must return the same bytes after every repeat; the exit status is 1 otherwise.
Separately, by device events, after the last repeat: rm_scene_tiles_device alone (option exact = 1) against
rm_scene_tiles_update_device alone over the same kept blocks, from the previous tiles and the last edit's balls, with the share
of blocks reused.  One JSON line per workload, merged into --out (a JSON object keyed by workload) when that is given."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from exact_bench import quartiles, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=("grid", "random1000", "c5"), required=True)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    N = R._native
    centers, radii, accel = workload(args.workload)
    full, sess = R.Context(0), R.Context(0)
    for c in (full, sess):
        c.scene_from_spheres(centers, radii, accel)
    c64 = centers.astype(np.float64)
    lo, hi = (c64 - radii[:, None]).min(axis=0), (c64 + radii[:, None]).max(axis=0)
    n = args.cells
    m = 2 * (hi - lo) / (n - 4)  # Context.mesh_box's margin for iso 0
    step = (hi - lo + 2 * m) / n
    geom = (lo - m, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), (n + 1,) * 3)
    session = sess.mesh_session(*geom)
    rng = np.random.default_rng(args.seed)
    cur = centers.copy()
    routes = {"full": lambda e: (full.edit_spheres(e), full.mesh_sparse(*geom, exact=True, order="tile", device=True))[1],
              "session": lambda e: (session.edit_spheres(e), session.mesh(order="tile", device=True))[1]}
    ms = {r: [] for r in routes}
    shares, same, balls = [], True, None
    for rep in range(args.warmup + args.reps):
        i = int(rng.integers(0, len(radii)))
        d = rng.normal(size=3)
        cur[i] = (cur[i].astype(np.float64) + 0.1 * float((hi - lo).max()) * d / np.linalg.norm(d)).astype(np.float32)
        edit = [("set", i, cur[i], float(radii[i]))]
        balls = sess.edit_balls(edit)
        last = {}
        for r in (("full", "session") if rep % 2 == 0 else ("session", "full")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[r] = routes[r](edit)
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ms[r].append(1e3 * (time.perf_counter() - t0))
        same = same and all(x.shape == y.shape and bool((x.view(torch.uint8) == y.view(torch.uint8)).all()) for x, y in zip(last["full"], last["session"]))
        if rep >= args.warmup:
            shares.append(session.stats["n_reused"] / max(1, session.stats["n_kept"]))

    # the two tile entries alone, by events, over the kept blocks of the last repeat
    lat, k = session.lattice, session.n_kept
    prev = session._sets[1 - session._cur]  # the set the last update copied from: still whole
    scratch = torch.empty((k, 729), dtype=torch.float64, device=session.slot.device)
    d_balls = torch.from_numpy(balls.view(np.uint8).reshape(-1).copy()).to(scratch.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def tiles_full():
        with sess._exact(True):
            N.check(sess._h, N.lib().rm_scene_tiles_device(sess._h, C.byref(lat), p(session.list), k, p(scratch), stream))

    def tiles_update():
        N.check(sess._h, N.lib().rm_scene_tiles_update_device(sess._h, C.byref(lat), p(prev[0]), p(prev[2]), prev[3], p(d_balls), len(balls), p(session.list),
                                                             k, p(scratch), None, None, stream))

    entries = {"tiles_device": tiles_full, "tiles_update_device": tiles_update}
    ev = {r: [] for r in entries}
    for rep in range(args.warmup + args.reps):
        for r in (tuple(entries) if rep % 2 == 0 else tuple(entries)[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            entries[r]()
            b.record()
            torch.cuda.synchronize()
            same = same and bool((scratch == session.tiles).logical_or(scratch.isnan() & session.tiles.isnan()).all())
            if rep >= args.warmup:
                ev[r].append(a.elapsed_time(b))
    res = {"workload": args.workload, "spheres": int(len(radii)), "accel": "BVH" if accel == 2 else "Octree", "cells": args.cells, "reps": args.reps,
           "n_blocks": session.n_blocks, "n_kept": k, "same_bytes": same, "reused_share_median": round(float(np.median(shares)), 4),
           "reused_share_min": round(float(min(shares)), 4), "last_edit": dict(session.stats),
           "vertices": int(len(session.mesh(order="tile", device=True)[0]))}
    for r in routes:
        res[r] = quartiles(ms[r])
    for r in entries:
        res[r] = quartiles(ev[r])
    a, b = res["full"], res["session"]
    res["full_over_session"] = round(a["median_ms"] / b["median_ms"], 2)
    res["session_below_full_by_more_than_the_larger_iqr"] = bool(a["median_ms"] - b["median_ms"] > max(a["iqr_ms"], b["iqr_ms"]))
    res["tiles_over_update"] = round(res["tiles_device"]["median_ms"] / res["tiles_update_device"]["median_ms"], 2)
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
