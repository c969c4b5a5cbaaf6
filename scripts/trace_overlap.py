"""How many render kernels run at once, and how many workgroups per CU they ask for together, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 48 --warmup 12
    python scripts/trace_overlap.py DIR/.../*_kernel_trace.csv [--cus 256] [--match REGEX] [--skip-ms 0]

A persistent launch of the v2 wave loop brings `blocks_per_cu` workgroups per CU; launches on streams that share
a hardware queue run one after the other, so the number of kernels that overlap is bounded by GPU_MAX_HW_QUEUES.  The trace's
start and end stamps show the overlap that really happened (a counter pass would serialise the launches).  Reported, weighted
by time, over the part of the span from the first start to the last end of the matching kernels (after --skip-ms of it) in which
at least one of them runs:
  * the distribution of the number of matching kernels running at once;
  * the distribution of the workgroups per CU those kernels ask for together: grid threads / workgroup threads / CUs, summed
    over the kernels running, and the mean of that capped at what a CU holds (--fit: six of the wave loop's workgroups);
  * the hardware queues the kernels ran on, and their durations.
Reads the CSV only: no GPU, no library."""
import argparse
import csv
import re
import sys
from collections import Counter

DEFAULT_MATCH = r"render_kernel|rm_rtc_render|frames_kernel"


def read_kernels(path, match):
    """[(start_ns, end_ns, workgroups, workgroup_threads, queue_id, name)] of the rows whose Kernel_Name matches."""
    rx = re.compile(match)
    out = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            if not rx.search(name):
                continue
            wg = max(1, int(row["Workgroup_Size_X"])) * max(1, int(row.get("Workgroup_Size_Y") or 1)) * max(1, int(row.get("Workgroup_Size_Z") or 1))
            grid = max(1, int(row["Grid_Size_X"])) * max(1, int(row.get("Grid_Size_Y") or 1)) * max(1, int(row.get("Grid_Size_Z") or 1))
            out.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), grid // wg, wg, row.get("Queue_Id", "?"), name))
    return out


def weighted(kernels, cus, skip_ns=0):
    """(span_ns, {kernels at once: ns}, {workgroups per CU asked together, rounded to 0.5: ns}) by a sweep over the stamps."""
    if not kernels:
        return 0, {}, {}
    t_first = min(k[0] for k in kernels) + skip_ns
    events = []
    for s, e, groups, _, _, _ in kernels:
        s, e = max(s, t_first), max(e, t_first)
        if e > s:
            events.append((s, 1, groups))
            events.append((e, -1, -groups))
    events.sort(key=lambda ev: (ev[0], ev[1]))  # at one stamp an end comes before a start
    at_once, per_cu = Counter(), Counter()
    running = groups = 0
    prev = events[0][0] if events else t_first
    for t, d, g in events:
        if t > prev:
            at_once[running] += t - prev
            per_cu[round(2.0 * groups / cus) / 2.0] += t - prev
        running += d
        groups += g
        prev = t
    span = (events[-1][0] - events[0][0]) if events else 0
    return span, dict(at_once), dict(per_cu)


def report(kernels, cus, skip_ns=0, fit=6, out=sys.stdout):
    span, at_once, per_cu = weighted(kernels, cus, skip_ns)
    w = out.write
    w("%d matching kernels, span %.3f ms, %d CUs\n" % (len(kernels), span / 1e6, cus))
    if not span:
        return
    dur = sorted(k[1] - k[0] for k in kernels)
    w("kernel duration ms: min %.3f median %.3f max %.3f\n" % (dur[0] / 1e6, dur[len(dur) // 2] / 1e6, dur[-1] / 1e6))
    w("workgroups per launch: %s\n" % ", ".join("%d x %d" % (n, g) for g, n in sorted(Counter(k[2] for k in kernels).items())))
    w("hardware queues used: %d (%s)\n" % (len({k[4] for k in kernels}), ", ".join("%s: %d" % qn for qn in sorted(Counter(k[4] for k in kernels).items()))))
    busy = span - at_once.get(0, 0)  # the time at least one matching kernel runs (the rest: set-up, compiles, host work)
    w("at least one kernel runs %.3f ms (%.1f %% of the span)\n" % (busy / 1e6, 100.0 * busy / span))
    if not busy:
        return
    w("kernels at once, share of that time:\n")
    for n in sorted(k for k in at_once if k):
        w("  %2d  %5.1f %%\n" % (n, 100.0 * at_once[n] / busy))
    w("  mean %.2f, most %d\n" % (sum(n * t for n, t in at_once.items()) / busy, max(at_once)))
    w("workgroups per CU asked together, share of that time (a CU holds at most %d):\n" % fit)
    for n in sorted(k for k in per_cu if k):
        w("  %4.1f  %5.1f %%\n" % (n, 100.0 * per_cu[n] / busy))
    w("  mean asked %.2f, mean of min(asked, %d) %.2f\n" % (sum(n * t for n, t in per_cu.items()) / busy, fit,
                                                           sum(min(n, fit) * t for n, t in per_cu.items()) / busy))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csv", help="*_kernel_trace.csv of rocprofv3 --kernel-trace --output-format csv")
    ap.add_argument("--cus", type=int, default=256, help="compute units of the device (MI355X: 256)")
    ap.add_argument("--match", default=DEFAULT_MATCH, help="regular expression a kernel's name must match")
    ap.add_argument("--skip-ms", type=float, default=0.0, help="leave out this much after the first matching kernel starts (set-up, warm-up)")
    ap.add_argument("--fit", type=int, default=6, help="workgroups of the render kernel a CU holds (the v2 wave loop: 6)")
    args = ap.parse_args()
    report(read_kernels(args.csv, args.match), args.cus, int(args.skip_ms * 1e6), args.fit)


if __name__ == "__main__":
    main()
