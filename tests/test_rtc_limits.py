"""Uploaded expression forests at the limits the product names for them (tests/forests.py lists the limits and builds the
forests), and the rule that a scene kernel compiled at run time is never loaded when it spills a VGPR (csrc/rm_rtc.cpp;
profiles/r03/spill_exec_hazard.txt is why).

CPU: every limit forest lands on the side of its limit the generator says, as the library reports it; every listed
(forest, accel, marcher family, vec3.length) compiles for gfx950 either with zero spilled VGPRs in both kernels or ends in a
clean `refused:` -- the decision a device context takes at the first render.  The outcomes are written to
profiles/rtc_limits_compile.txt by `python tests/_rtc_compile_worker.py --profile` (the table there is a record, not an input).

GPU: every forest that uploads is rendered, queried for distances, marched and picked through whichever kernel that decision
leaves it with -- its own, or the interpreter's -- and every result is the oracle's, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import forests as F  # noqa: E402
from _rtc_compile_worker import ACCEL_NAMES, CASES, COMPILES, case_id, compile_all  # noqa: E402  (the compile assignment lives there)
from test_gpu_parity import assert_same  # noqa: E402
from test_ray_pick import expected_ids, hit_points, single_object_values  # noqa: E402
from test_ray_queries import _assert_frame  # noqa: E402
from test_rtc_specialiser import usage  # noqa: E402  (the one parser of the resource-usage remarks)

OTHER = "adaptive-step-v3"  # the marcher that stands for the family "other than the sphere tracer"

# Which side of its limit every forest lands on, as the library must report it.  source: rtc_source() != "" (a scene kernel
# may be compiled); leaves: RM_RTC_BVH_LEAVES of that source (None: the tree stays data); slots / vals / instr:
# rm_scene_get_info's `program`; upload False: RM_E_UNSUPPORTED from rm_scene_from_nodes.
EXPECT = {
    "objects_31": dict(source=True, objects=31, leaves=None),
    "objects_32": dict(source=True, objects=32, leaves=None),
    "objects_33_out": dict(source=False, objects=33),
    "instructions_512": dict(source=True, instr=512),
    "instructions_513_out": dict(source=False, instr=513),
    "bvh_leaves_8": dict(source=True, bvh_leaves=8, leaves=8),
    "bvh_leaves_9_out": dict(source=True, bvh_leaves=9, leaves=None),
    "repetition_among_many": dict(source=True, objects=12, leaves=None),
    "coincident": dict(source=True, objects=11, leaves=7),
    "slots_15": dict(source=True, slots=15),
    "slots_16_out": dict(upload=False),
    "values_16": dict(source=True, vals=16),
    "values_17_out": dict(upload=False),
    "lds_exact": dict(source=True, slots=12, vals=14, lds=65536),
    "lds_under": dict(source=True, slots=12, vals=13, lds=65536 - 8 * 256),
    "lds_over_out": dict(upload=False),
    "random_8": dict(source=True, objects=8),
    "random_16": dict(source=True, objects=16),
    "random_30": dict(source=True, objects=30),
    "plain_depth_6": dict(source=True, objects=1, pruned=True),
    "every_operator": dict(source=True, objects=4, leaves=None),
}
UPLOADS = [n for n, e in EXPECT.items() if e.get("upload", True)]
# Two decisions that do not depend on the machine: the 16-object forest spills hundreds of VGPRs in both kernels (refused), the
# 32 small objects fit (accepted).  Forests that end at exactly 256 VGPRs are decided by a handful of spills, and that count
# was seen to differ between two machines with the same toolchain (0 and 8 for one 7-object forest), so no such forest is
# pinned here: for those the rule is checked on whatever the compiler reports (assert_rule).
KNOWN = {("random_16", 2, False, False): "refused", ("objects_32", 2, False, False): "accepted"}


def upload(ctx, oracle, name, accel=2):
    """The forest through the oracle's flattening into rm_scene_from_nodes; returns the oracle's scene."""
    osc = oracle.OracleScene(accel=ACCEL_NAMES[accel], prims=F.limit_forests()[name])
    ctx.scene_from_nodes(*osc.nodes(), accel)
    return osc


# ------------------------------------------------------------------------------------------------------------ CPU tests

@pytest.fixture(scope="module")
def host_ctx(rm):
    ctx = rm.Context(None)
    yield ctx
    ctx.close()


def test_the_assignment_covers_every_cell_twice():
    assert len(set(CASES)) == len(CASES)
    for accel in (0, 1, 2):
        for other in (False, True):
            for sq in (False, True):
                assert sum(1 for c in CASES if c[1:] == (accel, other, sq)) >= 2, (accel, other, sq)
    assert set(EXPECT) == set(F.limit_forests())
    assert COMPILES == [n for n in UPLOADS if EXPECT[n]["source"]]


@pytest.mark.parametrize("name", list(EXPECT))
def test_limit_forests_land_on_their_side(rm, oracle, host_ctx, name):
    import re
    e = EXPECT[name]
    if not e.get("upload", True):
        with pytest.raises(rm.RmUnsupported):
            upload(host_ctx, oracle, name)
        return
    upload(host_ctx, oracle, name)
    info, src = host_ctx.scene_info(), host_ctx.rtc_source()
    assert (src != "") == e["source"], (name, len(src))
    # RM_PROG_MAX_SLOTS is 16, but the host accepts 15 slots at the most (it refuses at `slot + 1 >= 16`: a node at slot s may
    # write slot s + 1), so the sixteenth slot is never used; 16 pending values are accepted.  Conservative, and left so.
    assert 1 <= info["prog_slots"] <= 15 and 1 <= info["prog_vals"] <= 16
    assert (info["prog_slots"] * 12 + info["prog_vals"] * 8) * 256 <= 65536
    for key, field in (("objects", "n_prims"), ("instr", "prog_instructions"), ("slots", "prog_slots"), ("vals", "prog_vals"), ("bvh_leaves", "bvh_leaves")):
        if key in e:
            assert info[field] == e[key], (name, key, info)
    if "lds" in e:
        assert (info["prog_slots"] * 12 + info["prog_vals"] * 8) * 256 == e["lds"]
    if e["source"] and "leaves" in e:
        m = re.search(r"RM_RTC_BVH_LEAVES (\d+)", src)
        assert (int(m.group(1)) if m else None) == e["leaves"], (name, m and m.group(1))
    if e.get("pruned"):
        assert "bounded subtree" in src


def outcome_of(log, secs=0.0):
    """What a compile log says: the rule's word (`refused:` ahead of the remarks) and the compiler's remarks themselves."""
    return dict(refused=log.startswith("refused:"), first_line=log.split("\n")[0][:200], usage=usage(log), seconds=secs)


def assert_rule(o, what):
    """The rule, re-stated on the compiler's remarks: both kernels reported; refused exactly when one of them spills a VGPR,
    and then the first line names such a function and its count."""
    u = o["usage"]
    assert set(u) == {"rm_rtc_render", "rm_rtc_distance"}, (what, o["first_line"])
    spills = {fn: r["VGPRs Spill"] for fn, r in u.items()}
    assert o["refused"] == any(spills.values()), (what, o["first_line"], spills)
    if o["refused"]:
        fn = o["first_line"].split()[1]
        assert o["first_line"].startswith("refused: %s spills %d VGPRs" % (fn, spills[fn])) and spills[fn] > 0, (what, o["first_line"], spills)


@pytest.fixture(scope="module")
def outcomes(rm, oracle):
    """case -> outcome, every case compiled once (in worker processes: _rtc_compile_worker.py)."""
    why = rm.Context(None)
    why.scene_from_preset(17, 2)
    try:
        why.rtc_compile_check(2, False)
    except RuntimeError as e:
        if "libhiprtc" in str(e):
            pytest.skip(str(e))
        raise
    finally:
        why.close()
    return {case: outcome_of(*ls) for case, ls in compile_all(CASES).items()}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scene_kernels_compile_without_spills_or_are_refused(outcomes, case):
    """Never an unguarded spilling module, never a compile error."""
    o = outcomes[case]
    assert_rule(o, case)
    if case in KNOWN:
        assert o["refused"] == (KNOWN[case] == "refused"), (case, o["first_line"])
    assert o["seconds"] < 600


def test_both_branches_of_the_rule_are_exercised(outcomes):
    assert any(o["refused"] for o in outcomes.values())
    assert any(not o["refused"] and EXPECT[c[0]].get("objects", 0) >= 8 for c, o in outcomes.items())


# ------------------------------------------------------------------------------------------------------------ GPU tests

ANG, TIME = (0.25, -0.6), 700.0
SMALL_FRAME = {"random_30": (64, 40), "random_16": (96, 60), "instructions_512": (96, 60), "every_operator": (80, 50)}  # the oracle is the slow side


@pytest.fixture(scope="module")
def lctx(rm):
    """A context of its own: options set here never leak into other test modules."""
    ctx = rm.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def sctx(rm):
    """The single-object scenes of the object-id check: interpreter only."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    yield c
    c.close()


def _render(rm, ctx, nodes, accel, alg, W, H):
    sc = rm.Scene(ACCEL_NAMES[accel], ctx=ctx)
    sc.loadNodes(*nodes)
    sc.camera.setAngles(*ANG)
    bufs = (np.zeros(W * H, np.uint8), np.zeros(3 * W * H, np.uint8), np.zeros(W * H, np.uint16), np.zeros(W * H, np.uint16))
    rm.createRaymarcher(alg, None, None).runRaymarcher(sc, *bufs, W, H, TIME, 0, H)
    return bufs


DEAR = ("random_8", "random_16", "random_30", "every_operator", "instructions_512")  # 4 - 40 s a compile on the GPU machine's host


def _assert_served_by_the_rule(ctx, own_kernel, interpreter, what):
    """After a lookup of the active scene's kernel with `specialise` = 1: rm_rtc_status holds the log of the compile behind it
    (fresh or from the process-wide cache).  The decision is re-derived from the compiler's remarks in that log (assert_rule)
    and must be the path that served: the scene's own kernel, or the interpreter after a `refused:`.  -> "own" | "refused"."""
    done, failed, log = ctx.rtc_status()
    o = outcome_of(log)
    assert_rule(o, what)
    if o["refused"]:
        assert interpreter and not own_kernel and (done, failed) == (0, 1), (what, done, failed, o["first_line"])
        return "refused"
    assert own_kernel and not interpreter and (done, failed) == (1, 0), (what, done, failed, o["first_line"])
    return "own"


def _is_interpreter(k):
    return k.startswith("render_kernel<") and k.split(">")[0].endswith((", 2", ", 3"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", UPLOADS)
def test_limit_forests_render_as_the_oracle(rm, oracle, lctx, name):
    """Rotated camera, time != 0, None / BVH / Octree, the sphere tracer and adaptive-step-v3, hypot and sqrt: the interpreter
    kernels (`specialise` = 0) in every cell, with one- and four-wave workgroups (the LDS budget is met by the latter), and
    `specialise` = 1 in every cell, where rm_last_kernel must show the path the rule leaves for THAT compile -- rm_rtc_render
    when the compiler's remarks show no spilled VGPR, the interpreter with `refused:` when they show one.  All four buffers
    equal the oracle's either way."""
    W, H = SMALL_FRAME.get(name, (160, 100))
    forest = F.limit_forests()[name]
    block0 = lctx.get_option("v1_block")
    served = {}
    try:
        for sq in (False, True):
            oracle.lib().ro_set_length_mode(int(sq))
            lctx.set_option("length", int(sq))
            for accel in (0, 1, 2):
                osc = oracle.OracleScene(accel=ACCEL_NAMES[accel], prims=forest)
                osc.set_angles(*ANG)
                nodes = osc.nodes()
                for other in (False, True):
                    alg = OTHER if other else "sphere-tracer"
                    what = "%s %s %s %s" % (name, ACCEL_NAMES[accel], alg, "sqrt" if sq else "hypot")
                    want = osc.render(W, H, algorithm=alg, time=TIME)
                    lctx.set_option("specialise", 0)
                    for block in (64, 256):
                        lctx.set_option("v1_block", block)
                        got = _render(rm, lctx, nodes, accel, alg, W, H)
                        assert _is_interpreter(lctx.last_kernel()), (what, lctx.last_kernel())
                        assert_same(got, want, what + " interpreter, v1_block %d" % block)
                    lctx.set_option("specialise", 1)
                    got = _render(rm, lctx, nodes, accel, alg, W, H)
                    k = lctx.last_kernel()
                    assert_same(got, want, what + " specialise 1: " + k)
                    assert ("[length=sqrt]" in k) == sq, (what, k)
                    if not lctx.rtc_source():  # beyond 32 objects / 512 instructions: no scene kernel to compile
                        assert not EXPECT[name]["source"] and _is_interpreter(k), (what, k)
                        continue
                    served[what] = _assert_served_by_the_rule(lctx, k.startswith("rm_rtc_render<"), _is_interpreter(k), what + ": " + k)
                    if (accel, other, sq) == (2, False, False) and name not in DEAR:  # the entry point the CPU tests use, on this machine
                        log, _ = lctx.rtc_compile_check(accel, other, refused_ok=True)
                        assert log.startswith("refused:") == (served[what] == "refused"), (what, log.split("\n")[0])
        print("\n".join("%s: %s" % kv for kv in served.items()))
    finally:
        lctx.set_option("specialise", 1)
        lctx.set_option("length", 0)
        lctx.set_option("v1_block", block0)
        oracle.lib().ro_set_length_mode(0)


@pytest.mark.gpu
@pytest.mark.parametrize("specialise", [1, 0], ids=["specialised", "ahead-of-time"])
@pytest.mark.parametrize("name", UPLOADS)
def test_limit_forests_answer_distances_as_the_oracle(rm, oracle, lctx, name, specialise):
    """2 000 random points, then the same points walked onto the surface four times: after every walk every twentieth point
    against the oracle, distance and count, NaN == NaN."""
    rng = np.random.default_rng(7)
    lctx.set_option("specialise", specialise)
    try:
        osc = oracle.OracleScene(accel="BVH", prims=F.limit_forests()[name])
        sc = rm.Scene("BVH", ctx=lctx)
        sc.loadNodes(*osc.nodes())
        sc.updateTime(250.0)
        pts = rng.uniform(-1.6, 1.6, (2000, 3)).astype(np.float32)
        checked = 0
        for walk in range(5):
            d, c = sc.getDistances(pts)
            if walk == 0 and specialise and lctx.rtc_source():  # rm_rtc_distance answered, or distance_kernel<..., 2|3> after a refusal
                _assert_served_by_the_rule(lctx, lctx.rtc_status()[0] == 1, lctx.rtc_status()[1] == 1, name + " getDistances")
            elif walk == 0:
                assert lctx.rtc_status()[:2] == (0, 0), lctx.rtc_status()[:2]
            for k in range(0, len(pts), 20):  # (the oracle answers one point per call)
                wd, wc = osc.distance(pts[k], time=250.0)
                assert (d[k] == wd or (np.isnan(d[k]) and np.isnan(wd))) and c[k] == wc, (name, walk, k, d[k], wd, c[k], wc)
                checked += 1
            dirs = rng.normal(size=pts.shape)
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            pts = (pts + dirs * np.clip(np.nan_to_num(d), -1, 1)[:, None] * 0.9).astype(np.float32)
        assert checked == 500
    finally:
        lctx.set_option("specialise", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", UPLOADS)
def test_limit_forests_through_the_ray_queries(rm, oracle, lctx, sctx, name):
    """The frame of the render test as camera rays through rm_ray_march and rm_ray_pick (the ahead-of-time query kernels on
    the largest programs they will see): the oracle's frame; every id in range or -1, and at every hit the scene of that
    object alone attains the scene's distance."""
    W, H = SMALL_FRAME.get(name, (96, 60))
    forest = F.limit_forests()[name]
    n_obj = len(forest)
    for accel, alg in ((2, "sphere-tracer"), (0, OTHER), (1, "sphere-tracer")):
        osc = oracle.OracleScene(accel=ACCEL_NAMES[accel], prims=forest)
        osc.set_angles(*ANG)
        want = osc.render(W, H, algorithm=alg, time=TIME)
        lctx.scene_from_nodes(*osc.nodes(), accel)
        org, dirs = rm.camera_rays(W, H, *ANG)
        o = np.ascontiguousarray(np.broadcast_to(org, dirs.shape))
        what = "%s %s %s" % (name, ACCEL_NAMES[accel], alg)
        march = lctx.ray_march(o, dirs, alg, normal=True, time=TIME)
        assert lctx.last_kernel().startswith("cast_kernel<"), lctx.last_kernel()
        _assert_frame(march, want, what + " ray_march")
        pick = lctx.pick(o, dirs, alg, normal=True, time=TIME)
        assert lctx.last_kernel().startswith("pick_kernel<"), lctx.last_kernel()
        _assert_frame(pick[:4], want, what + " pick")
        t, obj = pick[0], pick[4]
        assert ((obj >= -1) & (obj < n_obj)).all(), what
        hit = t < 10
        assert (obj[~hit] == -1).all(), what
        if not hit.any():
            continue
        p = hit_points(o[hit], dirs[hit], t[hit])
        lctx.scene_set_time(TIME)
        D, _ = lctx.scene_distance(p)
        v = single_object_values(lctx, sctx, p, n_obj, TIME)
        bad = obj[hit] != expected_ids(D, v, n_obj)
        assert not bad.any(), (what, np.nonzero(bad)[0][:8], obj[hit][bad][:8])


@pytest.mark.gpu
@pytest.mark.parametrize("name", UPLOADS)
def test_limit_forests_render_the_same_bytes_every_time(rm, oracle, lctx, name):
    """Twice in a row and once on a second stream (a spilling kernel's symptom was run-to-run variation): the same bytes, and
    they are the oracle's."""
    import torch
    W, H = SMALL_FRAME.get(name, (160, 100))
    dev = torch.device("cuda:%d" % lctx.device)
    osc = oracle.OracleScene(accel="BVH", prims=F.limit_forests()[name])
    osc.set_angles(*ANG)
    want = osc.render(W, H, time=TIME)
    lctx.set_option("specialise", 1)
    sc = rm.Scene("BVH", ctx=lctx)
    sc.loadNodes(*osc.nodes())
    sc.camera.setAngles(*ANG)

    def frame(stream=None):
        b = (torch.zeros(W * H, dtype=torch.uint8, device=dev), torch.zeros(3 * W * H, dtype=torch.uint8, device=dev),
             torch.zeros(W * H, dtype=torch.int16, device=dev), torch.zeros(W * H, dtype=torch.int16, device=dev))
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            rm.SphereTracer().runRaymarcher(sc, *b, W, H, TIME)
        torch.cuda.synchronize(dev)
        return [b[0].cpu().numpy(), b[1].cpu().numpy(), b[2].cpu().numpy().view(np.uint16), b[3].cpu().numpy().view(np.uint16)]

    first, second, third = frame(), frame(), frame(torch.cuda.Stream(device=dev))
    assert_same(first, want, name + " first")
    assert_same(second, want, name + " second")
    assert_same(third, want, name + " second stream")

