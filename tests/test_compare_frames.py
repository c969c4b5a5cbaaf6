"""rm_compare_frames_device / rm_compare_frames / Context.compare_frames / Context.compare: two G-buffer sets of the same
frames, B against A.  Every expectation comes from the numpy model of tests/compare_model.py (written from the header's
definitions); every comparison is exact -- every field of every record, every byte of the image."""
import ctypes as C

import numpy as np
import pytest

import compare_model as M

PAIRS = ("depth", "normal", "sdf", "iters")
ELEMS = {"depth": 1, "normal": 3, "sdf": 1, "iters": 1}  # elements per pixel
ALL_MAPS = ("sdf", "iters", "depth", "normal", "surface", "none")
GUARD = 64  # pixels behind the image, records behind the statistics: must keep their 0xFF


def synth(seed, total, present=PAIRS):
    """Seeded random sets A and B of `total` pixels (numpy; None for a pair not in `present`).  A third of the pixels are equal
    on both sides, normals are (128,128,128) on either, both or neither side, and the first pixels hold the extremes."""
    rng = np.random.default_rng(seed)

    def side():
        return {"depth": rng.integers(0, 256, total, dtype=np.uint8), "normal": rng.integers(0, 256, 3 * total, dtype=np.uint8),
                "sdf": rng.integers(0, 65536, total, dtype=np.uint16), "iters": rng.integers(0, 65536, total, dtype=np.uint16)}

    a, b = side(), side()
    same = rng.random(total) < 0.33
    for name in PAIRS:
        mask = np.repeat(same, ELEMS[name])
        b[name][mask] = a[name][mask]
    for s, p in ((a, 0.3), (b, 0.3)):
        miss = np.repeat(rng.random(total) < p, 3)
        s["normal"][miss] = 128
    forced = [  # (sdf a, sdf b, depth a, depth b, normal a, normal b)
        (0, 65535, 0, 255, (128, 128, 128), (1, 2, 3)), (65535, 0, 255, 0, (9, 128, 128), (128, 128, 128)),
        (7, 7, 3, 3, (128, 128, 128), (128, 128, 128)), (1, 2, 10, 11, (0, 255, 128), (255, 0, 127))]
    for i, (sa, sb, da, db, na, nb) in enumerate(forced[:total]):
        a["sdf"][i], b["sdf"][i], a["depth"][i], b["depth"][i] = sa, sb, da, db
        a["iters"][i], b["iters"][i] = sb, sa
        a["normal"][3 * i:3 * i + 3], b["normal"][3 * i:3 * i + 3] = na, nb
    if total > 4:  # a pixel identical in all four buffers
        for name in PAIRS:
            b[name][5 * ELEMS[name] - ELEMS[name]:5 * ELEMS[name]] = a[name][5 * ELEMS[name] - ELEMS[name]:5 * ELEMS[name]]
    return tuple(a[n] if n in present else None for n in PAIRS), tuple(b[n] if n in present else None for n in PAIRS)


def to_dev(x, shift):
    """A CUDA tensor with x's bytes; shift: the tensor starts one element past its allocation."""
    import torch
    if x is None:
        return None
    t = torch.empty(x.size + 1, dtype=torch.int16 if x.dtype == np.uint16 else torch.uint8, device="cuda:0")
    view = t[1:] if shift else t[:-1]
    view.copy_(torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x))
    return view


class Out:
    """Image and statistics buffers pre-filled with 0xFF, a guard region behind each."""

    def __init__(self, total, n, shift=0):
        import torch
        self.total, self.n = total, n
        self._rgba = torch.full((4 * (total + GUARD) + 4,), 0xFF, dtype=torch.uint8, device="cuda:0")
        self.rgba = self._rgba[shift:shift + 4 * (total + GUARD)]  # shift 1: one byte past, 4: one pixel past the allocation
        self.stats = torch.full((128 * (n + GUARD),), 0xFF, dtype=torch.uint8, device="cuda:0")

    def check(self, ctx, want, what, image=True, stats=True):
        import torch
        torch.cuda.synchronize()
        recs, img = want
        rgba, raw = self.rgba.cpu().numpy(), self.stats.cpu().numpy()
        if image and img is not None:
            bad = int((rgba[:4 * self.total] != img).sum())
            assert bad == 0, "%s: %d image bytes differ" % (what, bad)
            assert (rgba[4 * self.total:] == 0xFF).all(), what + ": image written past the last frame"
        else:
            assert (rgba == 0xFF).all(), what + ": image written"
        if stats:
            got = ctx.decode_compare_stats(raw[:128 * self.n])
            assert len(got) == len(recs) == self.n
            for k, (g, w) in enumerate(zip(got, recs)):
                assert g == w, "%s: record %d: %s" % (what, k, {f: (g[f], w[f]) for f in g if g[f] != w[f]})
            assert (raw[128 * self.n:] == 0xFF).all(), what + ": statistics written past the last record"
        else:
            assert (raw == 0xFF).all(), what + ": statistics written"


def run(ctx, a, b, W, rows, n, map, gain, shift=0, stats=True, what=""):
    """One device call on buffers of their own against the model."""
    total = W * rows * n
    da, db = [to_dev(x, shift) for x in a], [to_dev(x, shift) for x in b]
    out = Out(total, n, shift=(1 if shift else 0))
    ctx.compare_frames(da, db, rgba=out.rgba if map != "none" else None, map=map, gain=gain, stats=out.stats if stats else None,
                       width=W, rows=rows, n_frames=n)
    out.check(ctx, M.compare_frames(a, b, W * rows, n, M.MAPS[map], gain), what or "%dx%dx%d %s gain %d" % (W, rows, n, map, gain),
              stats=stats)
    return out


@pytest.fixture(scope="module")
def cctx(rm):
    ctx = rm.Context(0)
    yield ctx
    ctx.close()


SHAPES = [(1, 1), (63, 1), (64, 1), (65, 1), (255, 1), (257, 1), (33, 9), (1000, 3), (130, 100)]

# ---------------------------------------------------------------------------------------- GPU, synthetic buffers


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_map_and_alignment(rm, cctx, shape, n):
    """Pixel counts around the 16-pixel group and the 64-lane wave, frames that start off every vector alignment (odd W * rows,
    n > 1), one frame of several workgroups (130 x 100), bases at and one element past an allocation: all five maps and NONE,
    gains 1, 5 and 255, records and image against the model, guards untouched."""
    W, rows = shape
    a, b = synth(W * 1000 + rows * 10 + n, W * rows * n)
    for k, map in enumerate(ALL_MAPS):
        for shift in (0, 1):
            run(cctx, a, b, W, rows, n, map, (1, 5, 255)[(k + shift) % 3], shift=shift)
    run(cctx, a, b, W, rows, n, "sdf", 5, stats=False)  # image only
    assert cctx.last_kernel() == "compare_kernel<0, false>"


@pytest.mark.gpu
def test_image_one_pixel_past_an_allocation(rm, cctx):
    """An image 4 bytes past its allocation: whole pixels, but no 16-byte store is aligned with the other buffers' groups."""
    W, rows, n = 33, 9, 3
    a, b = synth(77, W * rows * n)
    da, db = [to_dev(x, 0) for x in a], [to_dev(x, 0) for x in b]
    out = Out(W * rows * n, n, shift=4)
    cctx.compare_frames(da, db, rgba=out.rgba, map="iters", gain=5, stats=out.stats, width=W, rows=rows, n_frames=n)
    out.check(cctx, M.compare_frames(a, b, W * rows, n, M.MAPS["iters"], 5), "image one pixel past")


@pytest.mark.gpu
def test_every_absent_pair_combination(rm, cctx):
    """33 x 9 x 3 with every subset of the four pairs: the fields of an absent pair are 0; the map is one whose pair is there."""
    W, rows, n = 33, 9, 3
    for mask in range(16):
        present = tuple(p for k, p in enumerate(PAIRS) if mask >> k & 1)
        a, b = synth(500 + mask, W * rows * n, present)
        maps = ["none"] + [m for m in ("sdf", "iters", "depth") if m in present] + (["normal", "surface"] if "normal" in present else [])
        for map in maps:
            run(cctx, a, b, W, rows, n, map, 5, what="pairs %s map %s" % (present, map))
    got = cctx.decode_compare_stats(run(cctx, (None,) * 4, (None,) * 4, W, rows, n, "none", 5).stats[:128 * n])
    assert got == [dict(M.ZERO, pixels=W * rows)] * n


@pytest.mark.gpu
def test_identical_sets(rm, cctx):
    W, rows, n = 257, 3, 3
    a, _ = synth(9, W * rows * n)
    for map in ("sdf", "iters", "depth"):
        out = run(cctx, a, a, W, rows, n, map, 255)
        img = out.rgba.cpu().numpy()[:4 * W * rows * n].reshape(-1, 4)
        assert (img == (0, 0, 0, 255)).all()
        for r in cctx.decode_compare_stats(out.stats[:128 * n]):
            for f in ("depth_differs", "normal_differs", "counters_differ", "surface_only_a", "surface_only_b", "b_cheaper", "a_cheaper",
                      "max_abs_depth", "max_abs_normal", "sum_abs_depth"):
                assert r[f] == 0, (map, f, r)
            assert r["surface_a"] == r["surface_b"] > 0 and r["sum_sdf_a"] == r["sum_sdf_b"] > 0


@pytest.mark.gpu
def test_scratch_is_left_ready(rm):
    """Frames of several workgroups (130 x 100: partial records and a ticket counter per frame from the context's ring): the same
    call twice on one context, then twice on two streams in flight, then often enough that the ring comes round several
    times -- the same records as the model every time, so every counter was left at zero and no call met another's entries."""
    import torch
    W, rows, n = 130, 100, 3
    total = W * rows * n
    a, b = synth(31, total)
    want = M.compare_frames(a, b, W * rows, n, M.MAPS["depth"], 5)
    da, db = [to_dev(x, 0) for x in a], [to_dev(x, 0) for x in b]
    ctx = rm.Context(0)
    outs = []
    for rep in range(2):
        outs.append(Out(total, n))
        ctx.compare_frames(da, db, rgba=outs[-1].rgba, map="depth", gain=5, stats=outs[-1].stats, width=W, rows=rows, n_frames=n)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")]
    for rep in range(4):
        outs.append(Out(total, n))
        torch.cuda.synchronize()  # (the 0xFF fill ran on the default stream)
        with torch.cuda.stream(streams[rep % 2]):
            ctx.compare_frames(da, db, rgba=outs[-1].rgba, map="depth", gain=5, stats=outs[-1].stats, width=W, rows=rows, n_frames=n)
    big = torch.full((128 * n,), 0xFF, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for rep in range(700):  # 12 entries a call: the ring of 4 096 comes round twice
        with torch.cuda.stream(streams[rep % 2]):
            ctx.compare_frames(da, db, map="none", stats=big, width=W, rows=rows, n_frames=n)
    for k, out in enumerate(outs):
        out.check(ctx, want, "call %d" % k)
    assert ctx.decode_compare_stats(big) == want[0]
    ctx.close()


@pytest.mark.gpu
def test_batches_beyond_the_ring_and_lanes_with_several_groups(rm, cctx):
    """4 100 frames of 5 pixels: more frames than the context's ring has entries (one workgroup per frame: none is needed).
    1 025 frames of 4 200 pixels: one workgroup per frame again, 262 groups for 256 lanes, so lanes take a second group."""
    for W, rows, n in ((5, 1, 4100), (4200, 1, 1025)):
        a, b = synth(W + n, W * rows * n)
        run(cctx, a, b, W, rows, n, "sdf", 5)


@pytest.mark.gpu
def test_no_pixel_and_no_frame(rm, cctx):
    a, b = synth(3, 64)
    da, db = [to_dev(x, 0) for x in a], [to_dev(x, 0) for x in b]
    for W, rows in ((0, 7), (7, 0), (0, 0)):
        out = Out(0, 3)
        cctx.compare_frames(da, db, rgba=out.rgba, map="sdf", gain=5, stats=out.stats, width=W, rows=rows, n_frames=3)
        out.check(cctx, ([dict(M.ZERO)] * 3, None), "%d x %d" % (W, rows))
    out = Out(0, 0)
    cctx.compare_frames(da, db, rgba=out.rgba, map="sdf", gain=5, stats=out.stats, width=8, rows=8, n_frames=0)
    out.check(cctx, ([], None), "no frame")


@pytest.mark.gpu
def test_host_entry_equals_device_entry(rm, cctx):
    W, rows, n = 65, 7, 3
    a, b = synth(11, W * rows * n, ("depth", "normal", "sdf"))
    for map in ("normal", "none"):
        dev = run(cctx, a, b, W, rows, n, map, 5)
        rgba = np.full(4 * W * rows * n + 16, 0xFF, np.uint8)
        stats = np.full(128 * (n + 1), 0xFF, np.uint8)
        cctx.compare_frames(a, b, rgba=rgba if map != "none" else None, map=map, gain=5, stats=stats, width=W, rows=rows, n_frames=n)
        assert np.array_equal(stats[:128 * n], dev.stats.cpu().numpy()[:128 * n]) and (stats[128 * n:] == 0xFF).all()
        if map != "none":
            assert np.array_equal(rgba[:-16], dev.rgba.cpu().numpy()[:4 * W * rows * n]) and (rgba[-16:] == 0xFF).all()
        else:
            assert (rgba == 0xFF).all()
    stats = np.full(128 * 2, 0xFF, np.uint8)
    cctx.compare_frames(a, b, map="none", stats=stats, width=0, rows=4, n_frames=2)
    assert (stats == 0).all()


# ---------------------------------------------------------------------------------------- GPU, rendered


def make_job(N, W, H, preset, accel, algorithm="sphere-tracer", step=float("nan")):
    j = N.rm_job()
    j.width, j.height, j.y_start, j.y_end = W, H, 0, H
    j.algorithm = N.lib().rm_algorithm_from_string(algorithm.encode())
    j.scene_preset_index, j.acceleration_structure = preset, {"None": 0, "Octree": 1, "BVH": 2}[accel]
    j.overshoot_factor, j.step_size = float("nan"), step
    return j


@pytest.mark.gpu
def test_sphere_tracer_against_fixed_step(rm):
    """Preset 3, 64 x 64, BVH, four views of a sweep: the sphere tracer (A) against FixedStep with step 0.1 (B).  Records and
    image equal the model applied to the rendered buffers; the sums of A equal what the same render_frames call reports."""
    import torch
    from cpu_raymarcher_amd import _native as N
    W = H = 64
    n, total = 4, 4 * 64 * 64
    views = rm.sweep_views(0.1, 0.0, 0.0, 0.4, n=n)
    ctx = rm.Context(0)
    sets, accs = [], []
    for job in (make_job(N, W, H, 3, "BVH"), make_job(N, W, H, 3, "BVH", "fixed-step", 0.1)):
        g = (torch.empty(total, dtype=torch.uint8, device="cuda:0"), torch.empty(3 * total, dtype=torch.uint8, device="cuda:0"),
             torch.empty(total, dtype=torch.int16, device="cuda:0"), torch.empty(total, dtype=torch.int16, device="cuda:0"))
        acc = torch.empty(4 * n, dtype=torch.int64, device="cuda:0")
        ctx.render_frames(job, views, *g, diag=acc)
        sets.append(g)
        accs.append(ctx.decode_accs(acc))
    attached = torch.full((4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    ctx._attach_diag(attached)
    host = [tuple(x.cpu().numpy().view(np.uint16) if x.dtype == torch.int16 else x.cpu().numpy() for x in g) for g in sets]
    for map in ("depth", "surface"):
        out = Out(total, n)
        ctx.compare_frames(sets[0], sets[1], rgba=out.rgba, map=map, gain=5, stats=out.stats, width=W, rows=H, n_frames=n)
        assert ctx.last_kernel().startswith("compare_kernel<")
        out.check(ctx, M.compare_frames(host[0], host[1], W * H, n, M.MAPS[map], 5), "rendered, " + map)
    got = ctx.decode_compare_stats(out.stats[:128 * n])
    for k in range(n):
        assert (got[k]["sum_sdf_a"], got[k]["sum_iters_a"]) == (accs[0][k]["total_sdf"], accs[0][k]["total_iters"])
        assert (got[k]["sum_sdf_b"], got[k]["sum_iters_b"]) == (accs[1][k]["total_sdf"], accs[1][k]["total_iters"])
        assert got[k]["surface_a"] > 0 and got[k]["counters_differ"] > 0  # two marchers: a comparison, not two copies
    # not a render entry: the attached accumulator survived the compare calls and is taken by the next render
    assert attached.cpu().tolist() == [0x5A5A5A5A5A5A5A5A] * 4
    job = make_job(N, W, H, 3, "BVH")
    job.camera_pitch, job.camera_yaw = float(views[1][0]), float(views[1][1])
    ctx.render_tile(job, None, None, None, None, rgba=torch.empty(4 * W * H, dtype=torch.uint8, device="cuda:0"))
    torch.cuda.synchronize()
    assert ctx.decode_acc(attached) == {k: accs[0][1][k] for k in ("total_sdf", "total_iters", "max_sdf", "min_sdf")}
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_views", [True, False])
def test_context_compare_bvh_against_none(rm, with_views):
    """Context.compare: one marcher with the BVH (B) against no acceleration structure (A), as a sweep through render_frames and
    as one frame through render_tile, against the model on renders of the test's own."""
    import torch
    from cpu_raymarcher_amd import _native as N
    W = H = 64
    ctx = rm.Context(0)
    ja, jb = make_job(N, W, H, 3, "None"), make_job(N, W, H, 3, "BVH")
    views = rm.sweep_views(0.1, 0.0, 0.0, 0.4, n=4) if with_views else None
    for j in (ja, jb):
        j.camera_pitch, j.camera_yaw = 0.1, 0.4
    stats, rgba = ctx.compare(ja, jb, views=views, map="sdf", gain=5)
    n = 4 if with_views else 1
    assert len(stats) == n and tuple(rgba.shape) == (n, H, W, 4)
    # the model on renders of our own
    sets = []
    for job in (ja, jb):
        g = (torch.empty(n * W * H, dtype=torch.uint8, device="cuda:0"), torch.empty(3 * n * W * H, dtype=torch.uint8, device="cuda:0"),
             torch.empty(n * W * H, dtype=torch.int16, device="cuda:0"), torch.empty(n * W * H, dtype=torch.int16, device="cuda:0"))
        if with_views:
            ctx.render_frames(job, views, *g)
        else:
            ctx.render_tile(job, *g)
        torch.cuda.synchronize()
        sets.append(tuple(x.cpu().numpy().view(np.uint16) if x.dtype == torch.int16 else x.cpu().numpy() for x in g))
    want, img = M.compare_frames(sets[0], sets[1], W * H, n, M.MAPS["sdf"], 5)
    assert stats == want and np.array_equal(rgba.cpu().numpy().reshape(-1), img)
    for r in stats:
        assert r["counters_differ"] > 0 and r["sum_sdf_a"] != r["sum_sdf_b"]  # the BVH changes what a pixel costs
    with pytest.raises(ValueError):
        ctx.compare(ja, make_job(N, W, H, 4, "BVH"))
    ctx.close()


# ---------------------------------------------------------------------------------------- CPU


def test_struct_layout(rm):
    from cpu_raymarcher_amd import _native as N
    S = N.rm_compare_stats
    assert C.sizeof(S) == 128 and C.sizeof(N.rm_frame_set) == 32
    names = ("pixels", "sum_sdf_a", "sum_sdf_b", "sum_iters_a", "sum_iters_b", "sum_abs_depth", "surface_a", "surface_b", "surface_only_a",
             "surface_only_b", "depth_differs", "normal_differs", "counters_differ", "b_cheaper", "a_cheaper")
    assert [getattr(S, f).offset for f in names] == [8 * k for k in range(15)]
    assert S.max_abs_depth.offset == 120 and S.max_abs_normal.offset == 124
    assert tuple(f for f, _ in S._fields_) == M.FIELDS
    hdr = open(__file__.replace("tests/test_compare_frames.py", "include/rm_raymarch.h")).read()
    body = hdr[hdr.index("typedef struct rm_compare_stats {"):hdr.index("} rm_compare_stats;")]
    import re
    declared = [x.strip() for line in body.split("\n")[1:] for x in re.sub(r"/\*.*?\*/", "", line).replace("uint64_t", "").replace("uint32_t", "").split(";")[0].split(",")]
    assert tuple(x for x in declared if x) == M.FIELDS


def test_host_only_context_checks_arguments_first(rm):
    """Every refusal of the header, on a context without a device: the checks come before the device check.  Valid arguments:
    RM_E_NO_DEVICE, also for frames without a pixel."""
    from cpu_raymarcher_amd import _native as N
    L = N.lib()
    ctx = rm.Context(None)
    buf = np.zeros(4096, np.uint16)
    p = buf.ctypes.data
    full = N.rm_frame_set(p, p, p, p)
    img, st = C.c_void_p(p), C.c_void_p(p)

    def both(width, rows, n, a, b, map, gain, rgba, stats):
        ra = None if a is None else C.byref(a)
        rb = None if b is None else C.byref(b)
        d = L.rm_compare_frames_device(ctx._h, width, rows, n, ra, rb, map, gain, rgba, stats, None)
        h = L.rm_compare_frames(ctx._h, width, rows, n, ra, rb, map, gain, rgba, stats)
        assert d == h, (d, h)
        return d

    assert both(8, 8, 1, full, full, 0, 5, img, st) == N.RM_E_NO_DEVICE
    assert both(8, 8, 1, full, full, -1, 0, None, None) == N.RM_E_NO_DEVICE  # NONE: no gain, no image needed
    assert both(0, 8, 3, full, full, 0, 5, img, st) == N.RM_E_NO_DEVICE
    assert both(8, 8, 0, full, full, 0, 5, img, st) == N.RM_E_NO_DEVICE
    assert both(8, 8, 65535, full, full, 0, 5, img, st) == N.RM_E_NO_DEVICE
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
    for args in bad:
        assert both(*args) == N.RM_E_INVALID, args
        assert L.rm_last_error(ctx._h)
    assert L.rm_compare_frames_device(None, 8, 8, 1, C.byref(full), C.byref(full), 0, 5, img, st, None) == N.RM_E_INVALID
    z = np.zeros(64, np.uint8)
    with pytest.raises(N.RmError) as e:
        ctx.compare_frames((z, None, None, None), (z, None, None, None), rgba=np.zeros(256, np.uint8), map="depth", width=8, rows=8)
    assert e.value.code == N.RM_E_NO_DEVICE
    ctx.close()


def test_model_on_a_case_worked_by_hand():
    """The model itself, on three pixels worked out from the header by hand."""
    a = (np.array([0, 9, 200], np.uint8), np.array([128, 128, 128, 1, 2, 3, 128, 128, 127], np.uint8),
         np.array([0, 10, 65535], np.uint16), np.array([5, 5, 5], np.uint16))
    b = (np.array([255, 9, 100], np.uint8), np.array([1, 2, 3, 1, 2, 60, 128, 128, 128], np.uint8),
         np.array([65535, 10, 0], np.uint16), np.array([5, 6, 5], np.uint16))
    recs, img = M.compare_frames(a, b, 3, 1, M.MAPS["sdf"], 5)
    assert recs == [dict(pixels=3, sum_sdf_a=65545, sum_sdf_b=65545, sum_iters_a=15, sum_iters_b=16, sum_abs_depth=355, surface_a=2,
                         surface_b=2, surface_only_a=1, surface_only_b=1, depth_differs=2, normal_differs=3, counters_differ=3,
                         b_cheaper=1, a_cheaper=1, max_abs_depth=255, max_abs_normal=127)]
    assert img.reshape(-1, 4).tolist() == [[255, 0, 0, 255], [0, 0, 0, 255], [0, 255, 0, 255]]
    assert M.compare_frames(a, b, 3, 1, M.MAPS["normal"], 2)[1].reshape(-1, 4).tolist() == [[254, 254, 0, 255], [114, 114, 0, 255], [2, 2, 0, 255]]
    assert M.compare_frames(a, b, 3, 1, M.MAPS["surface"], 2)[1].reshape(-1, 4).tolist() == [[255, 0, 0, 255], [96, 96, 96, 255], [0, 255, 0, 255]]
    assert M.compare_frames(a, b, 3, 1, M.MAPS["iters"], 255)[1].reshape(-1, 4).tolist() == [[0, 0, 0, 255], [255, 0, 0, 255], [0, 0, 0, 255]]


def test_compare_kernels_spill_no_vgpr_and_use_no_scratch():
    """The eleven compare_kernel<MAP, STATS> instantiations on the compiler's own resource-usage listing (read as
    test_render_frames.py reads it for the frames kernels)."""
    import test_build_invariants as B
    if not B.os.path.exists(B.HIPCC) or B.shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = B.resource_usage((), "rm_frame_ops.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void compare_kernel<")}
    assert len(kernels) == 11, sorted(usage)
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
