"""A sequence of small frames: one rm_render_frames_device call against one call per frame, on one GPU.  Run each scene
under its own time limit, e.g.

    timeout -k 10 300 python scripts/frames_bench.py --scene grid
    timeout -k 10 300 python scripts/frames_bench.py --scene chicken

64 views of the analytics sweep (Camera.rotateCamera(0, 0.015) per frame) at 256 x 256, iteration heatmap and the fused
diagnostics per frame, Dense Sphere Grid (preset 3) or Chicken (preset 17) with the BVH, three ways:
  (a) batch      one Context.render_frames call (frames_kernel<...>);
  (b) per_frame  64 render_tile calls with `kernel` = 1, `specialise` = 0 on one stream: the same per-ray code launched frame
                 by frame -- the like-for-like baseline;
  (c) in_flight  64 render_tile calls with the library's defaults over 12 streams, with the options bench.py uses for frames
                 in flight (blocks_per_cu 1, lpt 0): the best a caller without the batch entry can do.
Times are HIP-event times of the whole sequence (median of --reps after --warmup; the three ways alternate inside every
repetition, so a drift of the machine hits all three); every way must give the same hash over all rgba bytes and all 64
accumulators.  Condition: (a) is no slower than (b), the margin being the spread (max - min) of (b)'s own samples.  One JSON
line per scene; exit status 1 when a hash differs or the condition fails."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENES = {"grid": 3, "chicken": 17}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scene", choices=sorted(SCENES), required=True)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--streams", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import cpu_raymarcher_amd as R
    from cpu_raymarcher_amd import _native as N
    from cpu_raymarcher_amd.host import _job

    n, W = args.views, args.size
    npx = W * W
    dev = torch.device("cuda:0")
    scene = R.Scene("BVH")
    scene.loadPreset(SCENES[args.scene])
    ctx = scene.ctx
    views = R.sweep_views(0.0, 0.0, 0.0, 0.015, n=n)
    shader = N.lib().rm_shader_from_string(b"iteration-heatmap")
    rgba = torch.zeros(4 * npx * n, dtype=torch.uint8, device=dev)
    acc = torch.zeros(4 * n, dtype=torch.int64, device=dev)
    frames = [rgba[4 * npx * k:4 * npx * (k + 1)] for k in range(n)]
    accs = [acc[4 * k:4 * (k + 1)] for k in range(n)]
    jobs = []
    for pitch, yaw, time in views:
        scene.camera.setAngles(pitch, yaw)
        jobs.append(_job(scene, W, W, time, 0, W, "sphere-tracer"))
    streams = [torch.cuda.Stream(device=dev) for _ in range(args.streams)]
    joins = [torch.cuda.Event() for _ in streams]
    kernels = {}

    def options(**kw):
        for k, v in kw.items():
            ctx.set_option(k, v)

    def batch():
        ctx.render_frames(jobs[0], views, None, None, None, None, rgba=rgba, shader=shader, diag=acc)
        kernels["batch"] = ctx.last_kernel()

    def per_frame():
        options(kernel=1, specialise=0)
        for k in range(n):
            ctx.render_tile(jobs[k], None, None, None, None, rgba=frames[k], shader=shader, diag=accs[k])
        kernels["per_frame"] = ctx.last_kernel()
        options(kernel=0, specialise=1)

    def in_flight():
        options(blocks_per_cu=1, lpt=0)
        main_stream = torch.cuda.current_stream(dev)
        fork = torch.cuda.Event()
        fork.record(main_stream)
        for s in streams:
            s.wait_event(fork)
        for k in range(n):
            with torch.cuda.stream(streams[k % len(streams)]):
                ctx.render_tile(jobs[k], None, None, None, None, rgba=frames[k], shader=shader, diag=accs[k])
        kernels["in_flight"] = ctx.last_kernel()
        for s, ev in zip(streams, joins):
            ev.record(s)
            main_stream.wait_event(ev)
        options(blocks_per_cu=blocks_per_cu, lpt=lpt)

    blocks_per_cu, lpt = ctx.get_option("blocks_per_cu"), ctx.get_option("lpt")
    ways = {"batch": batch, "per_frame": per_frame, "in_flight": in_flight}
    hashes, samples = {}, {name: [] for name in ways}
    for name, fn in ways.items():  # every way alone first: its hash over everything it wrote
        rgba.zero_()
        acc.zero_()
        fn()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        h.update(rgba.cpu().numpy().tobytes())
        h.update(acc.cpu().numpy().tobytes())
        hashes[name] = h.hexdigest()[:16]
    for rep in range(args.warmup + args.reps):
        for name, fn in ways.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= args.warmup:
                samples[name].append(a.elapsed_time(b))
    med = {name: float(np.median(v)) for name, v in samples.items()}
    spread_b = float(max(samples["per_frame"]) - min(samples["per_frame"]))
    first = ctx.decode_accs(acc)[0]
    res = {"scene": args.scene, "preset": SCENES[args.scene], "accel": "BVH", "views": n, "size": [W, W], "shader": "iteration-heatmap",
           "ms": med, "frames_per_s": {k: n / (v * 1e-3) for k, v in med.items()},
           "samples_ms": {k: [round(x, 4) for x in v] for k, v in samples.items()},
           "per_frame_spread_ms": spread_b, "batch_no_slower_than_per_frame": med["batch"] <= med["per_frame"] + spread_b,
           "kernels": kernels, "hashes": hashes, "same_hash": len(set(hashes.values())) == 1, "diagnostics_frame0": first,
           "in_flight_streams": len(streams), "in_flight_options": {"blocks_per_cu": 1, "lpt": 0}}
    print(json.dumps(res))
    if not (res["same_hash"] and res["batch_no_slower_than_per_frame"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
