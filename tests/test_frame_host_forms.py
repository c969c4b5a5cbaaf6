"""The host form of each operation on rendered frames against its device form: rm_compare_frames, rm_counter_hist,
rm_shade_ranged, rm_shade_lit, rm_shade and rm_shade_field.  The two forms share their checks, their argument block and their
launch; what differs is where the buffers are, so every comparison here is byte for byte, on synthetic buffers, and every output
buffer of a call carries guard bytes behind its payload (16 behind an image, one record behind records) that must keep their
0xFF: a host form that sized a buffer wrongly copies too little (the payload differs) or too much (the guard is written).
What the kernels compute is pinned by test_compare_frames.py, test_counter_hist.py, test_ray_light.py and test_scene_field.py."""
import ctypes as C

import numpy as np
import pytest

import hist_model as HM
import test_compare_frames as TC
import test_counter_hist as TH

GUARD = {"rgba": 16, "stats": 128, "hist": 2128}
PAIRS = TC.PAIRS
# width, rows, frames: the per-frame stride at its smallest; one pixel past the 256-lane workgroup; frames of several
# workgroups, which go through the context's rings (test_counter_hist.py's `big`)
SMALL = [(1, 1, 3), (257, 1, 2)]
RING = (256, 129, 2)
SHAPES = SMALL + [RING]
IDS = ["%dx%dx%d" % s for s in SHAPES]


def on_device(x):
    """The CUDA tensor with a numpy array's bytes (16- and 32-bit unsigned as signed); tuples element by element; None stays."""
    import torch
    if x is None:
        return None
    if isinstance(x, tuple):
        return tuple(on_device(y) for y in x)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(x.dtype)
    return torch.from_numpy(x.view(signed) if signed else x).to("cuda:0")


def both_forms(ctx, call, ins, outs, what=""):
    """call(ctx, ins, outs) once with numpy buffers and once with CUDA tensors.  ins: name -> array, tuple of arrays or None;
    outs: name -> payload bytes, (payload bytes, bytes of the buffer) for a buffer larger than what the call may write, or
    None for an output that is not passed.  Every output is pre-filled with 0xFF and has GUARD[name] bytes more than was
    said.  Returns the host outputs."""
    import torch
    room = {k: v[1] if isinstance(v, tuple) else v for k, v in outs.items()}
    outs = {k: v[0] if isinstance(v, tuple) else v for k, v in outs.items()}
    host = {k: None if r is None else np.full(r + GUARD[k], 0xFF, np.uint8) for k, r in room.items()}
    call(ctx, ins, host)
    dev = {k: None if v is None else torch.full((v.size,), 0xFF, dtype=torch.uint8, device="cuda:0") for k, v in host.items()}
    call(ctx, {k: on_device(v) for k, v in ins.items()}, dev)
    torch.cuda.synchronize()
    for k, p in outs.items():
        if p is None:
            continue
        assert (host[k][p:] == 0xFF).all(), "%s: the host form wrote behind the %d bytes of %s" % (what, p, k)
        got = dev[k].cpu().numpy()
        assert (got[p:] == 0xFF).all(), "%s: the device form wrote behind the %d bytes of %s" % (what, p, k)
        bad = np.nonzero(got != host[k])[0]
        assert bad.size == 0, "%s: %s differs between the forms in %d bytes, first at %d" % (what, k, bad.size, bad[0])
    return host


def written(buf, payload):
    return payload > 0 and (buf[:payload] != 0xFF).any()


# ---- the six operations as call(ctx, ins, outs)

def compare(W, rows, n, map="sdf", gain=5):
    return lambda ctx, i, o: ctx.compare_frames(i["a"], i["b"], rgba=o["rgba"], map=map, gain=gain, stats=o["stats"], width=W, rows=rows, n_frames=n)


def hist(W, rows, n, mask="all", shift=0, permille=(10, 990)):
    return lambda ctx, i, o: ctx.counter_hist(i["sdf"], i["iters"], normal=i["normal"], mask=mask, bin_shift=shift, percentiles=permille,
                                              hist=o["hist"], width=W, rows=rows, n_frames=n)


def ranged(W, rows, n, counter="sdf", lo=3, hi=300):
    return lambda ctx, i, o: ctx.shade_ranged(counter, i["values"], o["rgba"], hist=i["hist"], lo=lo, hi=hi, width=W, rows=rows, n_frames=n)


def lit(W, rows, n):
    return lambda ctx, i, o: ctx.shade_lit(i["depth"], i["normal"], i["lit"], i["ao"], o["rgba"], width=W, rows=rows, n_frames=n)


def shade(shader, W, H):
    return lambda ctx, i, o: ctx.shade(shader, W, H, i["depth"], i["normal"], i["sdf"], i["iters"], o["rgba"])


def field(map, **kw):
    return lambda ctx, i, o: ctx.shade_field(i["values"], rgba=o["rgba"], map=map, **kw)


def compare_ins(seed, total, present=PAIRS):
    a, b = TC.synth(seed, max(total, 16), present)  # (a buffer without elements has no address to pass)
    return dict(a=a, b=b)


def hist_ins(seed, total, sdf=True, iters=True, normal=True):
    s, i, nrm = TH.synth(seed, max(total, 16))
    return dict(sdf=s if sdf else None, iters=i if iters else None, normal=nrm if normal else None)


def lit_ins(seed, total):
    rng = np.random.default_rng(seed)
    g = TC.synth(seed, max(total, 16))[0]
    return dict(depth=g[0], normal=g[1], lit=rng.random(max(total, 16), dtype=np.float32), ao=rng.random(max(total, 16), dtype=np.float32))


def shade_ins(seed, total):
    g = TC.synth(seed, max(total, 16))[0]
    return dict(zip(PAIRS, g))


def field_ins(seed, n, map):
    rng = np.random.default_rng(seed)
    if map == "distance":
        v = rng.uniform(-3.0, 3.0, max(n, 16))
        v[:4] = (-0.5, 0.0, float("nan"), 2.5)  # (the zero line is white, 0xFF in every byte: not the only value)
        return dict(values=v[:n] if n else v)
    return dict(values=rng.integers(0, 40, max(n, 16), dtype=np.uint32)[:n or None])


@pytest.fixture(scope="module")
def fctx(rm):
    ctx = rm.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------------- GPU, synthetic buffers


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_compare_frames(rm, fctx, shape):
    W, rows, n = shape
    total = W * rows * n
    ins = compare_ins(100 + W, total)
    for map in ("sdf", "normal", "surface"):
        out = both_forms(fctx, compare(W, rows, n, map), ins, dict(rgba=4 * total, stats=128 * n), "compare %s %s" % (shape, map))
        assert written(out["rgba"], 4 * total) and written(out["stats"], 128 * n)
    both_forms(fctx, compare(W, rows, n, "iters"), ins, dict(rgba=4 * total, stats=None), "compare %s without records" % (shape,))
    # no map: the caller's image is neither staged nor copied back
    out = both_forms(fctx, compare(W, rows, n, "none"), ins, dict(rgba=(0, 4 * total), stats=128 * n), "compare %s map none" % (shape,))
    assert written(out["stats"], 128 * n)


@pytest.mark.gpu
@pytest.mark.parametrize("gone", PAIRS)
def test_compare_frames_with_a_pair_absent_on_both_sides(rm, fctx, gone):
    for W, rows, n in SMALL:
        total = W * rows * n
        ins = compare_ins(7 + W, total, tuple(p for p in PAIRS if p != gone))
        map = "iters" if gone == "sdf" else "sdf"
        for stats in (128 * n, None):
            both_forms(fctx, compare(W, rows, n, map), ins, dict(rgba=4 * total, stats=stats), "compare without %s" % gone)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_counter_hist(rm, fctx, shape):
    W, rows, n = shape
    total = W * rows * n
    cases = [(dict(), "all"), (dict(), "surface"), (dict(), "background"), (dict(sdf=False), "all"), (dict(iters=False), "surface")]
    for absent, mask in cases:
        out = both_forms(fctx, hist(W, rows, n, mask, shift=(0 if W == 1 else 3)), hist_ins(200 + W, total, **absent), dict(hist=2128 * n),
                         "hist %s %s %s" % (shape, mask, absent))
        assert written(out["hist"], 2128 * n)
        assert fctx.last_kernel() == ("hist_kernel<false>" if mask == "all" else "hist_kernel<true>")
    # the mask "all" passes no normal buffer to the kernel, whether or not the caller gives one
    given = both_forms(fctx, hist(W, rows, n, "all"), hist_ins(200 + W, total), dict(hist=2128 * n))
    absent = both_forms(fctx, hist(W, rows, n, "all"), hist_ins(200 + W, total, normal=False), dict(hist=2128 * n))
    assert np.array_equal(given["hist"], absent["hist"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL, ids=IDS[:2])
def test_shade_ranged_with_and_without_records(rm, fctx, shape):
    W, rows, n = shape
    total = W * rows * n
    data = hist_ins(300 + W, total)
    records = both_forms(fctx, hist(W, rows, n, "all"), data, dict(hist=2128 * n))["hist"][:2128 * n].copy()
    for counter in ("sdf", "iters"):
        for rec in (None, records):
            out = both_forms(fctx, ranged(W, rows, n, counter), dict(values=data[counter], hist=rec), dict(rgba=4 * total),
                             "ranged %s %s %s" % (shape, counter, "records" if rec is not None else "lo, hi"))
            assert written(out["rgba"], 4 * total) and fctx.last_kernel() == "shade_ranged_kernel"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL, ids=IDS[:2])
def test_shade_lit(rm, fctx, shape):
    W, rows, n = shape
    total = W * rows * n
    out = both_forms(fctx, lit(W, rows, n), lit_ins(400 + W, total), dict(rgba=4 * total), "lit %s" % (shape,))
    assert written(out["rgba"], 4 * total)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (1, 3), (257, 1), (129, 5)], ids=lambda s: "%dx%d" % s)
def test_shade(rm, fctx, size):
    W, H = size
    for shader in range(4):
        out = both_forms(fctx, shade(shader, W, H), shade_ins(500 + W, W * H), dict(rgba=4 * W * H), "shade %d %s" % (shader, size))
        assert written(out["rgba"], 4 * W * H)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 257, 4099])
def test_shade_field_with_both_maps(rm, fctx, n):
    for map, kw in (("distance", dict()), ("distance", dict(range=0.7, band=0.031, line=0.004)), ("count", dict(lo=3, hi=10)), ("count", dict(lo=5, hi=5))):
        out = both_forms(fctx, field(map, **kw), field_ins(600 + n, n, map), dict(rgba=4 * n), "field %s %s n %d" % (map, kw, n))
        assert written(out["rgba"], 4 * n) and fctx.last_kernel() == "shade_field_kernel"


@pytest.mark.gpu
def test_no_frame_leaves_every_output_as_it_is(rm, fctx):
    W, rows = 8, 8
    both_forms(fctx, compare(W, rows, 0), compare_ins(1, 64), dict(rgba=0, stats=0), "compare, no frame")
    both_forms(fctx, hist(W, rows, 0), hist_ins(2, 64), dict(hist=0), "hist, no frame")
    both_forms(fctx, ranged(W, rows, 0), dict(values=hist_ins(3, 64)["sdf"], hist=None), dict(rgba=0), "ranged, no frame")
    both_forms(fctx, lit(W, rows, 0), lit_ins(4, 64), dict(rgba=0), "lit, no frame")
    from cpu_raymarcher_amd.context import _ptr
    N = rm._native
    sh = N.rm_field_shade()
    sh.map, sh.range, sh.band, sh.line = 0, 2.0, 0.25, 0.02

    def no_value(ctx, i, o):  # (Context.shade_field takes the count from the values: no value is asked of the library itself)
        dev = not isinstance(o["rgba"], np.ndarray)
        fn = N.lib().rm_shade_field_device if dev else N.lib().rm_shade_field
        N.check(ctx._h, fn(ctx._h, C.byref(sh), 0, _ptr(i["values"]), _ptr(o["rgba"]), *((None,) if dev else ())))

    both_forms(fctx, no_value, field_ins(5, 16, "distance"), dict(rgba=0), "field, no value")


@pytest.mark.gpu
def test_frames_without_a_pixel(rm, fctx):
    """compare: all-zero records; hist: the empty records, which carry the shift; no image byte anywhere."""
    for W, rows in ((0, 4), (4, 0)):
        n = 2
        out = both_forms(fctx, compare(W, rows, n), compare_ins(1, 0), dict(rgba=0, stats=128 * n), "compare, no pixel")
        assert (out["stats"][:128 * n] == 0).all()
        out = both_forms(fctx, compare(W, rows, n, "none"), compare_ins(1, 0), dict(rgba=0, stats=None), "compare, no pixel, no records")
        for shift, mask in ((0, "all"), (5, "surface")):
            out = both_forms(fctx, hist(W, rows, n, mask, shift), hist_ins(2, 0), dict(hist=2128 * n), "hist, no pixel")
            got = fctx.decode_hists(out["hist"][:2128 * n])
            assert len(got) == n
            for frame in got:
                assert not HM.same(frame["sdf"], HM.zero(shift)) and not HM.same(frame["iters"], HM.zero(shift))
        both_forms(fctx, ranged(W, rows, n), dict(values=hist_ins(3, 0)["sdf"], hist=out["hist"][:2128 * n].copy()), dict(rgba=0), "ranged, no pixel")
        both_forms(fctx, lit(W, rows, n), lit_ins(4, 0), dict(rgba=0), "lit, no pixel")
        both_forms(fctx, shade(0, W, rows), shade_ins(5, 0), dict(rgba=0), "shade, no pixel")


@pytest.mark.gpu
def test_host_calls_of_growing_size_on_one_context(rm):
    """Per operation a context of its own: a small host call, a larger one that makes the scratch buffer grow, and the small one
    again, which must give what it gave the first time.  (Each step is checked against the device form as well.)"""
    small, large = (1, 1, 3), (257, 1, 2)

    def px(s):
        return s[0] * s[1] * s[2]

    rec = {}
    steps = {
        "compare": lambda s: (compare(*s, "normal"), compare_ins(s[0], px(s)), dict(rgba=4 * px(s), stats=128 * s[2])),
        "hist": lambda s: (hist(*s, "surface"), hist_ins(s[0], px(s)), dict(hist=2128 * s[2])),
        "ranged": lambda s: (ranged(*s), dict(values=hist_ins(s[0], px(s))["sdf"], hist=rec[s]), dict(rgba=4 * px(s))),
        "lit": lambda s: (lit(*s), lit_ins(s[0], px(s)), dict(rgba=4 * px(s))),
        "shade": lambda s: (shade(1, s[0], s[1] * s[2]), shade_ins(s[0], px(s)), dict(rgba=4 * px(s))),
        "field": lambda s: (field("distance"), field_ins(s[0], px(s), "distance"), dict(rgba=4 * px(s))),
    }
    for name, step in steps.items():
        ctx = rm.Context(0)
        runs = []
        for s in (small, large, small):
            if name == "hist":
                rec[s] = None
            call, ins, outs = step(s)
            runs.append(both_forms(ctx, call, ins, outs, "%s %s" % (name, s)))
            if name == "hist":
                rec[s] = runs[-1]["hist"][:2128 * s[2]].copy()
        for k in runs[0]:
            assert np.array_equal(runs[0][k], runs[2][k]), "%s: %s changed when the call was repeated" % (name, k)
        ctx.close()


# ---------------------------------------------------------------------------------------- CPU


def test_both_forms_return_the_same_code_on_a_host_only_context(rm):
    """The argument sets of the host-only tests of test_compare_frames.py, test_counter_hist.py, test_ray_light.py,
    test_scene_field.py and test_host_logic.py, each given to the device entry and to the host entry of its pair: one code."""
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    INVALID, NO_DEVICE = N.RM_E_INVALID, N.RM_E_NO_DEVICE
    buf = np.zeros(8192, np.uint16)
    p = buf.ctypes.data
    seen = {INVALID: 0, NO_DEVICE: 0}

    def same(name, args, want):
        d = getattr(L, name + "_device")(ctx._h, *args, None)
        h = getattr(L, name)(ctx._h, *args)
        assert d == h == want, (name, args, d, h, want)
        seen[want] += 1

    # rm_compare_frames (test_compare_frames.py)
    full = N.rm_frame_set(p, p, p, p)
    img, st = C.c_void_p(p), C.c_void_p(p)
    ok = [(8, 8, 1, full, full, 0, 5, img, st), (8, 8, 1, full, full, -1, 0, None, None), (0, 8, 3, full, full, 0, 5, img, st),
          (8, 8, 0, full, full, 0, 5, img, st), (8, 8, 65535, full, full, 0, 5, img, st)]
    bad = [
        (8, 8, 1, None, full, 0, 5, img, st), (8, 8, 1, full, None, 0, 5, img, st),
        (-1, 8, 1, full, full, 0, 5, img, st), (8, -1, 1, full, full, 0, 5, img, st), (8, 8, -1, full, full, 0, 5, img, st),
        (8, 8, 65536, full, full, 0, 5, img, st),
        (8, 8, 1, full, full, -2, 5, img, st), (8, 8, 1, full, full, 5, 5, img, st),
        (8, 8, 1, full, full, 0, 0, img, st), (8, 8, 1, full, full, 4, 256, img, st), (8, 8, 1, full, full, 2, -3, img, st),
        (8, 8, 1, full, full, 0, 5, None, st),
        (8, 8, 1, full, full, -1, 5, None, C.c_void_p(p + 4)),  # records not 8-byte aligned
    ]
    for k in range(4):  # a pair on one side only, either side
        for side in range(2):
            v = [p, p, p, p]
            v[k] = None
            one = N.rm_frame_set(*v)
            bad.append((8, 8, 1, one, full, -1, 5, None, st) if side == 0 else (8, 8, 1, full, one, -1, 5, None, st))
    for map, k in ((0, 2), (1, 3), (2, 0), (3, 1), (4, 1)):  # a map whose pair is absent on both sides
        v = [p, p, p, p]
        v[k] = None
        gone = N.rm_frame_set(*v)
        bad.append((8, 8, 1, gone, gone, map, 5, img, st))
    odd = N.rm_frame_set(p, p, p + 1, p)
    bad.append((8, 8, 1, odd, odd, -1, 5, None, st))
    for args, want in [(a, NO_DEVICE) for a in ok] + [(a, INVALID) for a in bad]:
        w, r, n, a, b = args[:5]
        same("rm_compare_frames", (w, r, n, None if a is None else C.byref(a), None if b is None else C.byref(b)) + args[5:], want)

    # rm_counter_hist and rm_shade_ranged (test_counter_hist.py)
    BIG = 65536  # 65536 x 65536 pixels > UINT32_MAX

    def hist_args(width=8, rows=8, n=1, sdf=p, iters=p, normal=p, mask=0, shift=0, lo=0, hi=1000, out=p):
        return (width, rows, n, sdf, iters, normal, mask, shift, lo, hi, out)

    def ranged_args(counter=0, width=8, rows=8, n=1, values=p, rec=None, lo=0, hi=10, rgba=p):
        return (counter, width, rows, n, values, rec, lo, hi, rgba)

    for kw in (dict(), dict(width=0), dict(n=0), dict(n=65535), dict(normal=None), dict(sdf=None), dict(iters=None), dict(mask=2), dict(shift=8),
               dict(lo=500, hi=500), dict(lo=1000, hi=1000), dict(width=65535, rows=65537)):
        same("rm_counter_hist", hist_args(**kw), NO_DEVICE)
    for kw in (dict(out=None), dict(sdf=None, iters=None), dict(width=-1), dict(rows=-1), dict(n=-1), dict(width=BIG, rows=BIG), dict(n=65536),
               dict(mask=-1), dict(mask=3), dict(mask=1, normal=None), dict(mask=2, normal=None), dict(shift=-1), dict(shift=9),
               dict(lo=-1), dict(hi=1001), dict(lo=600, hi=599), dict(sdf=p + 1), dict(iters=p + 1), dict(out=p + 4)):
        same("rm_counter_hist", hist_args(**kw), INVALID)
    for kw in (dict(), dict(counter=1), dict(width=0), dict(n=0), dict(lo=7, hi=7), dict(rec=p, lo=9, hi=3), dict(lo=0, hi=2 ** 32 - 1)):
        same("rm_shade_ranged", ranged_args(**kw), NO_DEVICE)
    for kw in (dict(rgba=None), dict(values=None), dict(counter=2), dict(counter=-1), dict(width=-1), dict(rows=-1), dict(n=-1),
               dict(width=BIG, rows=BIG), dict(n=65536), dict(lo=4, hi=3), dict(values=p + 1), dict(rec=p + 4)):
        same("rm_shade_ranged", ranged_args(**kw), INVALID)

    # rm_shade_lit (test_ray_light.py)
    a = C.c_void_p(p)
    odd = C.c_void_p(p + 2)
    for hole in range(5):
        args = [a] * 5
        args[hole] = None
        same("rm_shade_lit", (4, 4, 1, *args), INVALID)
    for size in ((-1, 4, 1), (4, -1, 1), (4, 4, -1), (4, 4, 65536)):
        same("rm_shade_lit", size + (a, a, a, a, a), INVALID)
    same("rm_shade_lit", (4, 4, 1, a, a, odd, a, a), INVALID)
    same("rm_shade_lit", (4, 4, 1, a, a, a, odd, a), INVALID)
    same("rm_shade_lit", (4, 4, 1, a, a, a, a, a), NO_DEVICE)
    same("rm_shade_lit", (0, 4, 1, a, a, a, a, a), NO_DEVICE)

    # rm_shade_field (test_scene_field.py)
    NAN, INF = float("nan"), float("inf")

    def sh(map=0, range=2.0, band=0.25, line=0.02, lo=0, hi=0, reserved=0):
        s = N.rm_field_shade()
        s.map, s.reserved, s.range, s.band, s.line, s.lo, s.hi = map, reserved, range, band, line, lo, hi
        return C.byref(s)

    val, rgba = C.c_void_p(p), C.c_void_p(p)
    for n in (8, 0):
        same("rm_shade_field", (None, n, val, rgba), INVALID)
        same("rm_shade_field", (sh(), n, None, rgba), INVALID)
        same("rm_shade_field", (sh(), n, val, None), INVALID)
        for kw in (dict(map=-1), dict(map=2), dict(reserved=1), dict(range=0.0), dict(range=-1.0), dict(range=NAN), dict(range=INF),
                   dict(band=0.0), dict(band=-0.25), dict(band=NAN), dict(band=INF), dict(line=-0.01), dict(line=NAN), dict(line=INF),
                   dict(map=1, lo=5, hi=4), dict(map=1, reserved=2)):
            same("rm_shade_field", (sh(**kw), n, val, rgba), INVALID)
        same("rm_shade_field", (sh(), n, C.c_void_p(p + 4), rgba), INVALID)
        same("rm_shade_field", (sh(map=1), n, C.c_void_p(p + 2), rgba), INVALID)
    same("rm_shade_field", (sh(), -1, val, rgba), INVALID)
    same("rm_shade_field", (sh(), 8, val, rgba), NO_DEVICE)
    same("rm_shade_field", (sh(line=0.0, lo=9, hi=1), 8, val, rgba), NO_DEVICE)
    same("rm_shade_field", (sh(map=1, range=NAN, band=-1.0, line=-1.0, lo=3, hi=3), 8, C.c_void_p(p + 4), rgba), NO_DEVICE)
    same("rm_shade_field", (sh(), 0, val, rgba), NO_DEVICE)

    # rm_shade (test_host_logic.py): the device check comes first in both forms
    five = (a, a, a, a, a)
    for args in ((0, 4, 4) + five, (0, -4, 4) + five, (0, 4, -4) + five, (0, 4, 4, None, a, a, a, a), (0, 4, 4, a, a, a, a, None)):
        same("rm_shade", args, NO_DEVICE)
        assert L.rm_last_error(ctx._h).decode() == "host-only context"
    assert seen[INVALID] > 100 and seen[NO_DEVICE] > 30
    for name, args in (("rm_compare_frames", (8, 8, 1, C.byref(full), C.byref(full), 0, 5, img, st)), ("rm_counter_hist", hist_args()),
                       ("rm_shade_ranged", ranged_args()), ("rm_shade_lit", (4, 4, 1) + five), ("rm_shade_field", (sh(), 8, val, rgba)),
                       ("rm_shade", (0, 4, 4) + five)):
        assert getattr(L, name)(None, *args) == getattr(L, name + "_device")(None, *args, None) == INVALID, name  # a null context
    ctx.close()
