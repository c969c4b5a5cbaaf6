"""The sparse mesher (rm_scene_blocks_device, rm_scene_tiles_device, rm_mesh_tiles_device; Context.mesh_sparse) against the dense
path of the same run (Context.mesh).  One GPU, one process.  Run each scene under its own time limit, e.g.

    timeout -k 10 300 python scripts/mesh_sparse_bench.py --scene grid
    timeout -k 10 300 python scripts/mesh_sparse_bench.py --scene spheres10k --sizes 128 256 --sparse-only 512

Scenes: grid (the Dense Grid, preset 3, BVH), spheres1k (1 000 random spheres, BVH), spheres10k (the 10 000 random spheres of
cpu_raymarcher_amd/synthetic.py, octree), smooth (preset 10, "Smooth Union", an expression program, BVH); each over 1.2 times the
root box (the volume of scripts/mesh_bench.py), --sizes points a side with both paths, --sparse-only sizes with the sparse path
alone (the dense path cannot hold them).  Per size, HIP events on torch's current stream, --warmup calls first, then the median
of --reps with the minimum and the maximum:
  dense         Context.mesh(device=True): sample the volume, counting call, read the totals, allocate, filling call
  sparse_tile   Context.mesh_sparse(order="tile", device=True): blocks, read n_kept, tiles, counting call, read, filling call
  sparse_dense  the same with order="dense": plus two sorts and the renaming of the vertices in torch
  blocks, tiles, mesh   the three entries alone, on buffers that already exist (mesh: the filling call with exact capacities)
n_kept / n_blocks, the vertex and quad counts, and one hash of (vertices, quads) per path: dense and sparse_dense must hash
alike; the exit status is 1 otherwise.  One JSON line per size."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from field_bench import event_ms  # noqa: E402
from mesh_bench import digest, stats  # noqa: E402


def load(R, name):
    from cpu_raymarcher_amd.synthetic import synthetic_spheres
    if name == "grid":
        scene = R.Scene("BVH")
        scene.loadPreset(3)
    elif name == "smooth":
        scene = R.Scene("BVH")
        scene.loadPreset(10)
    else:
        s = synthetic_spheres(1000 if name == "spheres1k" else 10000)
        scene = R.Scene("BVH" if name == "spheres1k" else "Octree")
        scene.loadSpheres(s[:, :3], s[:, 3])
    return scene


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", choices=("grid", "spheres1k", "spheres10k", "smooth"), required=True)
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--sparse-only", type=int, nargs="*", default=[])
    ap.add_argument("--lipschitz", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
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
    for size in list(args.sizes) + list(args.sparse_only):
        with_dense = size in args.sizes
        shape = (size, size, size)
        step = 2 * h / np.array(shape)
        lattice = (c - h + step / 2, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), shape)
        lat = R.make_lattice(*lattice)
        res = {"scene": args.scene, "shape": list(shape), "n": size ** 3, "lipschitz": args.lipschitz}
        got = {}
        runs = {"sparse_tile": lambda: got.__setitem__("tile", ctx.mesh_sparse(*lattice, lipschitz=args.lipschitz, order="tile", device=True)),
                "sparse_dense": lambda: got.__setitem__("sparse", ctx.mesh_sparse(*lattice, lipschitz=args.lipschitz, device=True))}
        if with_dense:
            runs["dense"] = lambda: got.__setitem__("dense", ctx.mesh(*lattice, device=True))
        # the three stages alone, on buffers made once
        blocks = ctx.sparse_blocks(*lattice, lipschitz=args.lipschitz, dist=False)
        k, n_blocks = blocks.n_kept, len(blocks.slot)
        d_list = blocks.list.contiguous()
        d_slot2, d_list2 = torch.empty_like(blocks.slot), torch.empty(n_blocks, dtype=torch.int32, device="cuda")
        d_sinfo, d_info = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
        tiles = torch.empty((max(k, 1), 729), dtype=torch.float64, device="cuda")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

        def run_blocks():
            N.check(ctx._h, N.lib().rm_scene_blocks_device(ctx._h, C.byref(lat), 0.0, args.lipschitz, p(d_slot2), p(d_list2), None, p(d_sinfo), None))

        def run_tiles():
            N.check(ctx._h, N.lib().rm_scene_tiles_device(ctx._h, C.byref(lat), p(d_list), k, p(tiles), None))

        def run_mesh(v, cv, q, cq):
            N.check(ctx._h, N.lib().rm_mesh_tiles_device(ctx._h, C.byref(lat), p(blocks.slot), p(d_list), k, p(tiles), 0.0, p(v), cv, p(q), cq, None, None,
                                                         p(d_info), None))
        with torch.cuda.stream(torch.cuda.default_stream()):
            run_tiles()
            run_mesh(None, 0, None, 0)
            torch.cuda.synchronize()
            V, Q, holes = (int(x) for x in d_info.cpu()[:3])
            out_v, out_q = torch.empty((V, 3), dtype=torch.float32, device="cuda"), torch.empty((Q, 4), dtype=torch.int32, device="cuda")
            runs.update(blocks=run_blocks, tiles=run_tiles, mesh=lambda: run_mesh(out_v if V else None, V, out_q if Q else None, Q))
            times = {name: [] for name in runs}
            for rep in range(args.warmup + args.reps):  # the figures alternate inside a repetition
                for name, fn in runs.items():
                    ms = event_ms(torch, fn)
                    if rep >= args.warmup:
                        times[name].append(ms)
        for name in runs:
            res[name] = stats(times[name])
        res.update(n_blocks=n_blocks, n_kept=k, kept_fraction=round(k / max(n_blocks, 1), 4), vertices=V, quads=Q, holes=holes)
        res["hash_sparse"] = digest(*got["sparse"])
        res["hash_tile"] = digest(*got["tile"])
        res["tile_is_the_entries"] = res["hash_tile"] == digest(out_v, out_q)
        ok = ok and res["tile_is_the_entries"]
        if with_dense:
            res["hash_dense"] = digest(*got["dense"])
            res["same_hash"] = res["hash_dense"] == res["hash_sparse"]
            res["sparse_tile_vs_dense"] = round(res["sparse_tile"]["ms"] / res["dense"]["ms"], 3)
            res["sparse_dense_vs_dense"] = round(res["sparse_dense"]["ms"] / res["dense"]["ms"], 3)
            ok = ok and res["same_hash"]
        print(json.dumps(res), flush=True)
        del got, tiles, out_v, out_q, blocks
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
