"""Ray-query throughput (rm_ray_march_device, cast_kernel<...>) on one GPU.  Run each step under its own time limit, e.g.

    timeout -k 10 300 python scripts/ray_bench.py --case C3
    timeout -k 10 300 python scripts/ray_bench.py --case C5

C3: the 3840 x 2160 camera rays of the Dense Sphere Grid (BVH, angles 0.2 / 0.5) in two orders -- row order and 8 x 8-tile
order (the wave tiles of the one-ray-per-lane render) -- against the `kernel` = 1 render of the same frame, which runs the
same per-ray code.  C5: 1 M random rays from inside the octree cube through the 10 000-sphere scene.
Times are HIP-event kernel times (median of --reps launches after --warmup); every variant must give the same hash
(the depth / normal bytes and the u16 counters, in pixel order).  One JSON line per case.

--walk measures the walk query (rm_ray_walk_device, walk_kernel<...>) on the same rays instead: the march without normals
(what a walk marches), the summaries-only walk and the traced walk at cap 200, outputs allocated once (the traced C3 frame
holds 8.3 M x 200 x 24 B = 39.8 GB of records).  With RM_HIP_LIB naming an older build of the library that has no walk
entries, only the march is timed: the figure to put beside the walk's.  The summaries must carry the march's t, iterations
and SDF calls, traced or not."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def frame_hash(depth, normal, sdf, iters):
    h = hashlib.sha256()
    for b in (depth, normal, sdf, iters):
        h.update(np.ascontiguousarray(b).tobytes())
    return h.hexdigest()[:16]


def query_bytes(R, out, order=None):
    """rayMarch outputs -> the render's four buffers (depth byte, normal bytes, u16 counters), back in pixel order."""
    t, it, sdf, nrm = (x.cpu().numpy() for x in out)
    if order is not None:
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))
        t, it, sdf, nrm = t[inv], it[inv], sdf[inv], nrm[inv]
    depth = np.where(np.isnan(t), 0, np.clip(np.rint(t), 0, 255)).astype(np.uint8)
    n = (nrm.astype(np.float64) + 1) * 0.5 * 255
    normal = np.where(np.isnan(n), 0, np.clip(np.rint(n), 0, 255)).astype(np.uint8).reshape(-1)
    return depth, normal, (sdf.view(np.uint32) & 0xFFFF).astype(np.uint16), (it.view(np.uint32) & 0xFFFF).astype(np.uint16)


def walk_case(R, torch, args, ctx, res, sets):
    """--walk: for every (name, origins, directions) of `sets` the march without normals, the summaries-only walk and the
    traced walk at cap 200 through the device entries."""
    import ctypes as C
    N = R._native
    L = N.lib()
    have_walk = hasattr(L, "rm_ray_walk_device")
    cap = 200
    q = N.rm_ray_query()
    q.algorithm, q.normal, q.time = 0, 0, 0.0
    q.overshoot_factor = q.step_size = float("nan")
    ok = True
    for name, og, dg in sets:
        n = og.shape[0]
        out = [None]

        def march():
            out[0] = ctx.ray_march(og, dg, normal=False)
        res["march_%s_ms" % name] = timed(torch, march, args.warmup, args.reps)
        res["march_%s_per_s" % name] = n / (res["march_%s_ms" % name] * 1e-3)
        res["march_kernel"] = ctx.last_kernel()
        if not have_walk:
            continue
        t, it, sdf = (x.cpu().numpy() for x in out[0][:3])
        walks = torch.empty((n, 48), dtype=torch.uint8, device="cuda")
        for label, steps in (("walk", None), ("trace", torch.empty(n * cap * 24, dtype=torch.uint8, device="cuda"))):
            sp = C.c_void_p(steps.data_ptr()) if steps is not None else None

            def run():
                N.check(ctx._h, L.rm_ray_walk_device(ctx._h, C.byref(q), n, C.c_void_p(og.data_ptr()), C.c_void_p(dg.data_ptr()),
                                                     cap if steps is not None else 0, C.c_void_p(walks.data_ptr()), sp,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            walks.zero_()
            res["%s_%s_ms" % (label, name)] = timed(torch, run, args.warmup, args.reps)
            res["%s_%s_per_s" % (label, name)] = n / (res["%s_%s_ms" % (label, name)] * 1e-3)
            res["%s_%s_vs_march" % (label, name)] = res["%s_%s_ms" % (label, name)] / res["march_%s_ms" % name]
            w = walks.cpu().numpy().view(N.WALK_DTYPE).reshape(-1)
            ok = ok and w["t"].tobytes() == t.tobytes() and np.array_equal(w["evals"], it.view(np.uint32)) and \
                np.array_equal(w["sdf_calls"], sdf.view(np.uint32))
            if steps is not None:
                res["records_%s" % name] = int(w["evals"].astype(np.int64).sum() + w["skips"].sum())
            del steps
        res["walk_kernel"] = ctx.last_kernel()
    res["same_hash"] = ok  # (the summaries carry the march's numbers)
    return res


def case_c3(R, torch, args):
    W, H, ang = 3840, 2160, (0.2, 0.5)
    scene = R.Scene("BVH")
    scene.loadPreset(3)
    scene.camera.setAngles(*ang)
    ctx = scene.ctx
    res = {"case": "C3 rays", "rays": W * H}
    if args.walk:
        org, dirs = R.camera_rays(W, H, *ang)
        y, x = np.divmod(np.arange(W * H), W)
        sets = []
        for name, order in (("row", None), ("tile8x8", np.lexsort((x % 8, y % 8, x // 8, y // 8)))):
            d = dirs if order is None else dirs[order]
            sets.append((name, torch.from_numpy(np.broadcast_to(org, d.shape).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()))
        return walk_case(R, torch, args, ctx, res, sets)
    # the kernel = 1 render of the same frame
    ctx.set_option("kernel", 1)
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    render = lambda: R.SphereTracer().runRaymarcher(scene, *bufs, W, H, 0.0)  # noqa: E731
    res["render_kernel1_ms"] = timed(torch, render, args.warmup, args.reps)
    res["render_kernel"] = ctx.last_kernel()
    hashes = {"render_kernel1": frame_hash(bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), bufs[2].cpu().numpy().view(np.uint16),
                                           bufs[3].cpu().numpy().view(np.uint16))}
    ctx.set_option("kernel", 0)
    org, dirs = R.camera_rays(W, H, *ang)
    y, x = np.divmod(np.arange(W * H), W)
    orders = {"row": None, "tile8x8": np.lexsort((x % 8, y % 8, x // 8, y // 8))}
    for name, order in orders.items():
        d = dirs if order is None else dirs[order]
        og = torch.from_numpy(np.broadcast_to(org, d.shape).copy()).cuda()
        dg = torch.from_numpy(np.ascontiguousarray(d)).cuda()
        out = [None]

        def run():
            out[0] = ctx.ray_march(og, dg)
        res["rays_%s_ms" % name] = timed(torch, run, args.warmup, args.reps)
        res["rays_%s_per_s" % name] = W * H / (res["rays_%s_ms" % name] * 1e-3)
        hashes["rays_" + name] = frame_hash(*query_bytes(R, out[0], order))
    res["kernel"] = ctx.last_kernel()
    res["hashes"] = hashes
    res["same_hash"] = len(set(hashes.values())) == 1
    res["tile_vs_render"] = res["rays_tile8x8_ms"] / res["render_kernel1_ms"]
    return res


def case_c5(R, torch, args):
    from cpu_raymarcher_amd.synthetic import synthetic_spheres
    scene = R.Scene("Octree")
    sp = synthetic_spheres(10000)
    scene.loadSpheres(sp[:, :3], sp[:, 3])
    ctx = scene.ctx
    n = 1 << 20
    x = np.uint64(0x5EED)  # splitmix64
    vals = np.empty(6 * n, np.uint64)
    with np.errstate(over="ignore"):
        k = np.arange(1, 6 * n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + x
        z = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        vals[:] = z ^ (z >> np.uint64(31))
    u = (vals >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    o = (u[:3 * n].reshape(n, 3) * 19.5 - 9.75).astype(np.float32)
    d = (u[3 * n:].reshape(n, 3) * 2 - 1).astype(np.float32)
    og, dg = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    out = [None]

    def run():
        out[0] = ctx.ray_march(og, dg)
    res = {"case": "C5 rays", "rays": n}
    if args.walk:
        return walk_case(R, torch, args, ctx, res, [("random", og, dg)])
    res["rays_ms"] = timed(torch, run, args.warmup, args.reps)
    res["rays_per_s"] = n / (res["rays_ms"] * 1e-3)
    res["kernel"] = ctx.last_kernel()
    first = frame_hash(*query_bytes(R, out[0]))
    ctx.set_option("filter", 0)  # a second variant: the unfiltered leaf scans (same values)
    scene.loadSpheres(sp[:, :3], sp[:, 3])
    run()
    torch.cuda.synchronize()
    res["hashes"] = {"default": first, "filter0": frame_hash(*query_bytes(R, out[0]))}
    res["same_hash"] = res["hashes"]["default"] == res["hashes"]["filter0"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=("C3", "C5"), required=True)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--walk", action="store_true", help="time the walk query (summaries only, and traced at cap 200) beside the march")
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    res = (case_c3 if args.case == "C3" else case_c5)(R, torch, args)
    print(json.dumps(res))
    if not res["same_hash"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
