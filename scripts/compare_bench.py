"""rm_compare_frames_device against the code that moved the same bytes before it existed.

At 3840 x 2160 with all four pairs, map SDF and statistics on, the compare launch reads 16 B and writes 4 B per pixel.  The
yardstick moves the same 20 B per pixel over the same buffers with the entries the library already had: one rm_shade_device
(8 B read, 4 B written) and two rm_reduce_counters_enqueue (4 B read each).  HIP-event times, 5 warm-up rounds, then 10
rounds in which the two alternate; medians, ranges and the achieved GB/s of each.  Condition: the compare launch is no slower
than the yardstick plus the spread (max - min) of the yardstick's own ten samples.

Also: 64 frames of 256 x 256 in one call against 64 single-frame calls.

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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    import cpu_raymarcher_amd as R
    from cpu_raymarcher_amd import _native
    if not torch.cuda.is_available():
        raise SystemExit("compare_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    ctx = R.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def sets(total):
        out = []
        for _ in range(2):
            out.append((torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g),
                        torch.randint(0, 256, (3 * total,), dtype=torch.uint8, device=dev, generator=g),
                        torch.randint(-32768, 32768, (total,), dtype=torch.int16, device=dev, generator=g),
                        torch.randint(0, 300, (total,), dtype=torch.int16, device=dev, generator=g)))
        return out

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3  # us

    W, H = args.width, args.height
    total = W * H
    A, B = sets(total)
    rgba = torch.empty(4 * total, dtype=torch.uint8, device=dev)
    stats = torch.empty(128, dtype=torch.uint8, device=dev)
    acc = torch.empty(8, dtype=torch.int64, device=dev)

    def compare():
        ctx.compare_frames(A, B, rgba=rgba, map="sdf", gain=5, stats=stats, width=W, rows=H, n_frames=1)

    def yardstick():  # 8 + 4 + 4 B read, 4 B written per pixel, over the same buffers
        ctx.shade(2, W, H, A[0], A[1], A[2], A[3], rgba)
        ctx.reduce_counters_enqueue(B[2], B[3], acc[:4])
        ctx.reduce_counters_enqueue(A[2], A[3], acc[4:])

    for _ in range(args.warmup):
        compare()
        yardstick()
    torch.cuda.synchronize()
    t_cmp, t_yard = [], []
    for _ in range(args.rounds):
        t_cmp.append(timed(compare))
        t_yard.append(timed(yardstick))
    compare()
    kernel = ctx.last_kernel()
    gb = 20.0 * total / 1e9

    def summary(t):
        med = statistics.median(t)
        return {"median_us": round(med, 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "gb_per_s": round(gb / (med * 1e-6), 1)}

    spread = max(t_yard) - min(t_yard)
    res = {"size": [W, H], "bytes_per_pixel": 20, "kernel": kernel, "compare": summary(t_cmp), "yardstick": summary(t_yard),
           "yardstick_spread_us": round(spread, 2),
           "no_slower_than_yardstick_plus_spread": statistics.median(t_cmp) <= statistics.median(t_yard) + spread}

    # 64 frames of 256 x 256: one call against 64 calls
    n, w = 64, 256
    A, B = sets(n * w * w)
    rgba = torch.empty(4 * n * w * w, dtype=torch.uint8, device=dev)
    stats = torch.empty(128 * n, dtype=torch.uint8, device=dev)
    npx = w * w
    singles = [([x[k * npx * e:(k + 1) * npx * e] for x, e in zip(A, (1, 3, 1, 1))], [x[k * npx * e:(k + 1) * npx * e] for x, e in zip(B, (1, 3, 1, 1))],
                rgba[4 * k * npx:4 * (k + 1) * npx], stats[128 * k:128 * (k + 1)]) for k in range(n)]

    def batch():
        ctx.compare_frames(A, B, rgba=rgba, map="sdf", gain=5, stats=stats, width=w, rows=w, n_frames=n)

    def one_by_one():
        for a, b, img, st in singles:
            ctx.compare_frames(a, b, rgba=img, map="sdf", gain=5, stats=st, width=w, rows=w, n_frames=1)

    for _ in range(args.warmup):
        batch()
        one_by_one()
    torch.cuda.synchronize()
    t_batch, t_single = [], []
    for _ in range(args.rounds):
        t_batch.append(timed(batch))
        t_single.append(timed(one_by_one))
    res["frames_64x256x256"] = {"one_call_us": round(statistics.median(t_batch), 2), "one_call_range_us": [round(min(t_batch), 2), round(max(t_batch), 2)],
                                "64_calls_us": round(statistics.median(t_single), 2), "64_calls_range_us": [round(min(t_single), 2), round(max(t_single), 2)]}
    res["lib"] = os.path.basename(_native.LIB_PATH)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
