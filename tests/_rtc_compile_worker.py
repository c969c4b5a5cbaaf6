"""The compile assignment of test_rtc_limits.py and its worker: one rm_rtc_compile_check (hiprtc for gfx950, no GPU) of one limit
forest per process, so that the test can run a few at a time.

  python tests/_rtc_compile_worker.py --case '["random_8", 2, false, false]'   prints the compiler's log and the seconds as JSON
  python tests/_rtc_compile_worker.py --profile                                  rewrites profiles/rtc_limits_compile.txt"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ACCEL_NAMES = {0: "None", 1: "Octree", 2: "BVH"}
# forests of tests/forests.py that upload and have a specialised source (test_limit_forests_land_on_their_side asserts both)
COMPILES = ["objects_31", "objects_32", "instructions_512", "bvh_leaves_8", "bvh_leaves_9_out", "repetition_among_many", "coincident", "slots_15", "values_16",
            "lds_exact", "lds_under", "random_8", "random_16", "random_30", "plain_depth_6", "every_operator"]
# The compile assignment, fixed: every forest with a source under (BVH, sphere tracer, hypot); every other cell of
# accel {0, 1, 2} x family {sphere tracer, other} x length {hypot, sqrt} for two or three forests (the cheaper ones: the
# 16- and 30-object forests take 16 - 120 s a compile).  (accel, other, sqrt) -> forests.
MAIN = (2, False, False)
SPREAD = {
    (0, False, False): ("random_8", "coincident"),
    (0, True, False): ("random_8", "bvh_leaves_8"),
    (2, True, False): ("random_8", "values_16"),
    (1, False, False): ("objects_31", "slots_15"),
    (1, True, False): ("lds_exact", "repetition_among_many"),
    (2, False, True): ("lds_exact", "plain_depth_6", "every_operator"),
    (2, True, True): ("coincident", "lds_under"),
    (0, False, True): ("random_8", "values_16"),
    (0, True, True): ("objects_32", "bvh_leaves_9_out"),
    (1, False, True): ("instructions_512", "coincident"),
    (1, True, True): ("slots_15", "bvh_leaves_8"),
}
CASES = [(n,) + MAIN for n in COMPILES] + [(n,) + cell for cell, names in SPREAD.items() for n in names]


def case_id(c):
    return "%s-%s-%s-%s" % (c[0], ACCEL_NAMES[c[1]], "other" if c[2] else "tracer", "sqrt" if c[3] else "hypot")


def compile_case(name, accel, other, sq):
    """One rm_rtc_compile_check on a host-only context -> (log, seconds)."""
    import cpu_raymarcher_amd as R
    from oracle import oracle as O
    import forests as F
    ctx = R.Context(None)
    try:
        ctx.set_option("length", int(sq))
        osc = O.OracleScene(accel=ACCEL_NAMES[accel], prims=F.limit_forests()[name])
        ctx.scene_from_nodes(*osc.nodes(), accel)
        return ctx.rtc_compile_check(accel, other, refused_ok=True)
    finally:
        ctx.close()


def compile_all(cases):
    """case -> (log, seconds), every case in a process of its own, a few at a time (one hiprtc compile is one thread, and the
    largest forest alone takes one to two minutes), the dearest first so that the pool ends together."""
    def run(case):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", json.dumps(case)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
        assert out.returncode == 0, (case, out.stderr.decode()[-2000:])
        log, secs = json.loads(out.stdout.decode().split("\n__CASE__\n")[1])
        return log, secs

    order = sorted(cases, key=lambda c: -{"random_30": 9, "random_16": 8, "random_8": 7, "instructions_512": 6, "every_operator": 5}.get(c[0], 0))
    with ThreadPoolExecutor(max_workers=max(1, min(6, len(os.sched_getaffinity(0))))) as pool:
        return dict(zip(order, pool.map(run, order)))


def write_profile(path):
    """profiles/rtc_limits_compile.txt: the outcome of every case, for whoever tunes the generator or the specialiser next."""
    from test_rtc_specialiser import usage  # (the one parser of the resource-usage remarks)
    done = compile_all(CASES)
    rows = ["# tests/test_rtc_limits.py, the listed compile assignment: rm_rtc_compile_check (hiprtc, gfx950) on a host-only context",
            "# forest accel family length | outcome | rm_rtc_render VGPRs spill scratch[B/lane] waves/SIMD | rm_rtc_distance ... | seconds (six compiles at a time)"]
    for case in CASES:
        log, secs = done[case]
        u = usage(log)
        cols = ["%d %d %d %d" % (r["VGPRs"], r["VGPRs Spill"], r["ScratchSize [bytes/lane]"], r["Occupancy [waves/SIMD]"])
                for r in (u["rm_rtc_render"], u["rm_rtc_distance"])]
        rows.append("%-22s %-6s %-6s %-5s | %-8s | %-16s | %-16s | %.1f" % (case[0], ACCEL_NAMES[case[1]], "other" if case[2] else "tracer", "sqrt" if case[3] else "hypot",
                                                                            "refused" if log.startswith("refused:") else "accepted", cols[0], cols[1], secs))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        print("\n__CASE__\n" + json.dumps(compile_case(*json.loads(sys.argv[2]))))
    elif sys.argv[1:] == ["--profile"]:
        write_profile(os.path.join(ROOT, "profiles", "rtc_limits_compile.txt"))
    else:
        sys.exit(__doc__)
