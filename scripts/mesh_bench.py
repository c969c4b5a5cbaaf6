"""Mesh extraction (rm_mesh_field_device: mesh_count / mesh_scan / mesh_vertex / mesh_quad kernels) against the sampling that
feeds it and against the route a host had before: download the volume.  One GPU.  Run each step under its own time limit, e.g.

    timeout -k 10 300 python scripts/mesh_bench.py --scene grid
    timeout -k 10 300 python scripts/mesh_bench.py --scene spheres

Two scenes -- the Dense Grid (preset 3) under the BVH and the 10 000 random spheres of cpu_raymarcher_amd/synthetic.py under the
octree --, each as a 128^3 and a 256^3 volume over 1.2 times the root box (the volume of scripts/field_bench.py).  All from one
run:
  (a) mesh      rm_mesh_field_device on the resident binary64 volume with exact capacities: HIP-event time of the call (four
                kernels); `count` the counting call (mesh_count + mesh_scan alone), `mesh32` the same on the binary32 volume
  (s) sample    rm_scene_field_device writing dist (f64) alone: HIP-event time -- what (a) is to be read against
  (b) scene     Context.mesh(device=True): sample, counting call, read the totals, allocate, filling call; wall time, it
                ends in a synchronise
  (c) download  rm_scene_field of dist32 into a numpy array, wall time: what a host paid before it could start meshing
Warm-up calls first, then --reps timed ones; every figure is the median with the minimum and the maximum beside it.  The
meshes of (a) and (b) must hash alike; the exit status is 1 otherwise.  One JSON line per workload."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from field_bench import event_ms, load, wall_ms  # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).view(np.uint8).tobytes())
    return h.hexdigest()[:16]


def stats(ms):
    ms = sorted(ms)
    return {"ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", choices=("grid", "spheres"), required=True)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    N = R._native
    scene = load(R, args.scene)
    ctx = scene.ctx
    info = scene.info()
    mn, mx = np.array(info["root_min"]), np.array(info["root_max"])
    c, h = (mn + mx) / 2, 1.2 * (mx - mn) / 2
    ok = True
    for size in args.sizes:
        shape = (size, size, size)
        n = size ** 3
        step = 2 * h / np.array(shape)
        origin, du, dv, dw = c - h + step / 2, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2])
        lat = R.make_lattice(origin, du, dv, dw, shape)
        res = {"scene": args.scene, "shape": list(shape), "n": n}
        vol = {}

        def sample():
            vol["f64"], _ = ctx.field(origin, du, dv, dw, shape=shape, count=False, device=True)
        sample()
        vol["f32"] = vol["f64"].to(torch.float32)
        d_info = torch.zeros(4, dtype=torch.int64, device="cuda")

        def entry(values, vt, vertices, cap_v, quads, cap_q):
            N.check(ctx._h, N.lib().rm_mesh_field_device(ctx._h, C.byref(lat), C.c_void_p(values.data_ptr()), vt, 0.0,
                                                         None if vertices is None else C.c_void_p(vertices.data_ptr()), cap_v,
                                                         None if quads is None else C.c_void_p(quads.data_ptr()), cap_q,
                                                         C.c_void_p(d_info.data_ptr()), None))
        with torch.cuda.stream(torch.cuda.default_stream()):
            entry(vol["f64"], N.RM_MESH_F64, None, 0, None, 0)
            torch.cuda.synchronize()
            V, Q, holes = (int(x) for x in d_info.cpu()[:3])
            out = {k: (torch.empty((V, 3), dtype=torch.float32, device="cuda"), torch.empty((Q, 4), dtype=torch.int32, device="cuda")) for k in ("f64", "f32")}
            runs = {"mesh": lambda: entry(vol["f64"], N.RM_MESH_F64, out["f64"][0], V, out["f64"][1], Q),
                    "count": lambda: entry(vol["f64"], N.RM_MESH_F64, None, 0, None, 0),
                    "mesh32": lambda: entry(vol["f32"], N.RM_MESH_F32, out["f32"][0], V, out["f32"][1], Q),
                    "sample": sample}
            times = {k: [] for k in runs}
            for rep in range(args.warmup + args.reps):  # the figures alternate inside a repetition
                for k, fn in runs.items():
                    ms = event_ms(torch, fn)
                    if rep >= args.warmup:
                        times[k].append(ms)
        for k in runs:
            res[k] = stats(times[k])
        res["vertices"], res["quads"], res["holes"] = V, Q, holes
        res["hash"] = digest(*out["f64"])
        res["hash32"] = digest(*out["f32"])
        got = {}

        def whole():
            got["mesh"] = ctx.mesh(origin, du, dv, dw, shape, device=True)
        whole()
        res["scene_mesh"] = stats([wall_ms(torch, whole) for _ in range(args.reps)])
        res["same_hash"] = digest(*got["mesh"]) == res["hash"]

        def download():
            got["vol"] = ctx.field(origin, du, dv, dw, shape=shape, dist32=True, count=False)
        download()
        res["download"] = stats([wall_ms(torch, download) for _ in range(args.host_reps)])
        res["download_bytes"] = int(got["vol"][0].nbytes)
        res["mesh_vs_sample"] = round(res["mesh"]["ms"] / res["sample"]["ms"], 3)
        res["download_vs_scene_mesh"] = round(res["download"]["ms"] / res["scene_mesh"]["ms"], 2)
        print(json.dumps(res), flush=True)
        ok = ok and res["same_hash"]
        del vol, out, got
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
