"""rm_counter_hist_device and rm_shade_ranged_device against the entries that read the same bytes before they existed.

One C3 frame (Dense Sphere Grid, BVH, sphere tracer) at 3840 x 2160 is rendered once; its two counter buffers (4 B per pixel)
and its normals then go through
  * rm_reduce_counters_enqueue                         the yardstick of the histogram: the same 4 B per pixel
  * rm_counter_hist_device, mask all, shift 0 and 8    (4 B per pixel)
  * rm_counter_hist_device, mask surface, shift 0      (7 B per pixel: the normals too)
  * rm_counter_hist_device, mask all, on a CONSTANT frame (every pixel one value: the same-address path)
  * rm_shade_device, iteration heatmap                 the yardstick of the ranged shade (8 B read, 4 B written)
  * rm_shade_ranged_device from the histogram's record (2 B read, 4 B written)
HIP-event times of single launches, 5 warm-up rounds, then `--rounds` rounds in which all of them alternate; medians, ranges
(max - min, the run-to-run spread) in microseconds.  No threshold: the figures go to profiles/NOTES.md.

Prints one JSON line.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    import cpu_raymarcher_amd as R
    from cpu_raymarcher_amd import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("hist_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    ctx = R.Context(0)
    W, H = args.width, args.height
    total = W * H
    job = N.rm_job()
    job.width, job.height, job.y_start, job.y_end = W, H, 0, H
    job.algorithm = N.lib().rm_algorithm_from_string(b"sphere-tracer")
    job.scene_preset_index, job.acceleration_structure = 3, 2
    job.camera_pitch, job.camera_yaw = 0.2, 0.5
    job.overshoot_factor = job.step_size = float("nan")
    depth = torch.empty(total, dtype=torch.uint8, device=dev)
    normal = torch.empty(3 * total, dtype=torch.uint8, device=dev)
    sdf = torch.empty(total, dtype=torch.int16, device=dev)
    iters = torch.empty(total, dtype=torch.int16, device=dev)
    ctx.render_tile(job, depth, normal, sdf, iters)
    const_s, const_i = torch.full_like(sdf, 7), torch.zeros_like(iters)
    rgba = torch.empty(4 * total, dtype=torch.uint8, device=dev)
    hist = torch.empty(2128, dtype=torch.uint8, device=dev)
    acc = torch.empty(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def h(s, i, mask, shift):
        return lambda: ctx.counter_hist(s, i, normal=normal, mask=mask, bin_shift=shift, percentiles=(0, 990), hist=hist, width=W, rows=H)

    cases = {
        "reduce_counters_enqueue": lambda: ctx.reduce_counters_enqueue(sdf, iters, acc),
        "hist_all_shift0": h(sdf, iters, "all", 0),
        "hist_all_shift8": h(sdf, iters, "all", 8),
        "hist_surface_shift0": h(sdf, iters, "surface", 0),
        "hist_all_constant_frame": h(const_s, const_i, "all", 0),
        "reduce_counters_enqueue_constant_frame": lambda: ctx.reduce_counters_enqueue(const_s, const_i, acc),
        "shade_iteration_heatmap": lambda: ctx.shade(3, W, H, depth, normal, sdf, iters, rgba),
        "shade_ranged_from_record": lambda: ctx.shade_ranged("iters", iters, rgba, hist=hist, width=W, rows=H),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3  # us

    samples = {k: [] for k in cases}
    for rnd in range(args.warmup + args.rounds):
        for name, fn in cases.items():
            t = timed(fn)
            if rnd >= args.warmup:
                samples[name].append(t)
    rec = ctx.decode_hists(hist)[0]["iters"]
    out = {"width": W, "height": H, "rounds": args.rounds, "unit": "us",
           "surface_share": float((normal.view(-1, 3) != 128).any(dim=1).float().mean()),
           "iters_record": {k: v for k, v in rec.items() if k != "bins"}}
    for name, v in samples.items():
        out[name] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                     "spread": round(max(v) - min(v), 2)}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
