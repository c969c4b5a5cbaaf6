"""From how many work items per wave does a launch gain by bringing more workgroups per CU than the floor of `min_fill`?
(option `overlap_fill`, RM_V2_OVERLAP_ITEMS_PER_WAVE in csrc/rm_kernels.h; scripts/size_scaling.py is the model.)

C3 at 3840 x H for several H, S frames in flight with bench.py's in-flight options, the hardware queues as the environment has
them.  Per H the configurations `blocks_per_cu` = floor and = candidate (with `min_fill` 0: exactly that many) are alternated
`rounds` times; a line per run, then per H the ranges and whether the candidate's slowest run beats the floor's fastest.
usage: python scripts/fill_threshold.py [floor=2] [candidate=4] [rounds=3] [S=12] [frames=96] [H=270,540,...] [opt=value ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cpu_raymarcher_amd as R


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    floor, cand = int(kv.pop("floor", 2)), int(kv.pop("candidate", 4))
    rounds, S, frames = int(kv.pop("rounds", 3)), int(kv.pop("S", 12)), int(kv.pop("frames", 96))
    heights = [int(h) for h in kv.pop("H", "270,540,810,1080,1620,2160").split(",")]
    dev = torch.device("cuda:0")
    ctx = R.Context(0)
    for k, v in dict(item_px=256, tile_w=8, lpt=0, min_fill=0, **{k: int(v) for k, v in kv.items()}).items():
        ctx.set_option(k, v)
    cus = ctx.last_launch()["cus"]
    sc = R.Scene("BVH", ctx=ctx)
    sc.loadPreset(3)
    tr = R.SphereTracer()
    streams = [torch.cuda.Stream() for _ in range(S)]
    W = 3840
    print("GPU_MAX_HW_QUEUES=%s, %d CUs, %d frames in flight, floor %d, candidate %d workgroups per CU" %
          (os.environ.get("GPU_MAX_HW_QUEUES"), cus, S, floor, cand), flush=True)
    for H in heights:
        sets = [dict(d=torch.zeros(W * H, dtype=torch.uint8, device=dev), n=torch.zeros(3 * W * H, dtype=torch.uint8, device=dev),
                     s=torch.zeros(W * H, dtype=torch.int16, device=dev), i=torch.zeros(W * H, dtype=torch.int16, device=dev),
                     r=torch.zeros(4 * W * H, dtype=torch.uint8, device=dev), acc=torch.zeros(4, dtype=torch.int64, device=dev)) for _ in range(S)]

        def run(n):
            for f in range(n):
                b = sets[f % S]
                with torch.cuda.stream(streams[f % S]):
                    tr.runRaymarcher(sc, b["d"], b["n"], b["s"], b["i"], W, H, 0.0, shadedBuffer=b["r"], shader="iteration-heatmap", diagnostics=b["acc"])

        items = (W // 8) * -(-H // 32)
        got = {floor: [], cand: []}
        run(2 * S)  # the set-up frames; the wave loop compiled for this frame size takes over here
        torch.cuda.synchronize()
        for r in range(rounds):
            for per_cu in (floor, cand):
                ctx.set_option("blocks_per_cu", per_cu)
                run(S)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(frames)
                torch.cuda.synchronize()
                fps = frames / (time.perf_counter() - t0)
                got[per_cu].append(fps)
                wg = ctx.last_launch()["workgroups"]
                print("H %4d round %d per_cu %d: %8.1f frames/s  %d workgroups, %.2f items per wave" % (H, r + 1, per_cu, fps, wg, items / (4.0 * wg)), flush=True)
        f0, f1, c0, c1 = min(got[floor]), max(got[floor]), min(got[cand]), max(got[cand])
        print("H %4d: %5d items, %.2f per wave of the candidate | floor %.1f - %.1f | candidate %.1f - %.1f | slowest candidate / fastest floor %+.1f %%"
              % (H, items, items / (4.0 * min((items + 3) // 4, cus * cand)), f0, f1, c0, c1, 100.0 * (c0 / f1 - 1.0)), flush=True)
        del sets


if __name__ == "__main__":
    main()
