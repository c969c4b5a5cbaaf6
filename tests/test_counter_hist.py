"""rm_counter_hist_device / rm_counter_hist / rm_shade_ranged_device / rm_shade_ranged, Context.counter_hist / decode_hists /
shade_ranged, percentile and the two ranged heatmap models of host.py.  Every expectation comes from the numpy model of
tests/hist_model.py (written from the header's definitions); every comparison is exact -- every field of every record, every
byte of every image."""
import ctypes as C

import numpy as np
import pytest

import hist_model as M

GUARD = 64  # pixels behind the image, records behind the records: must keep their 0xFF
REC = 2128
EXTREMES = (0, 254, 255, 256, 65535)
PERMILLES = ((0, 1000), (500, 500), (10, 990))


def synth(seed, total, kind="random"):
    """(sdf, iters, normal) of `total` pixels.  random: seeded, half of the values small and half over the whole u16 range, 40 %
    of the normals (128,128,128), the extremes forced into the first pixels; constant: every pixel one value (the contention
    path); runs: two values in runs of 1 .. 700 pixels."""
    rng = np.random.default_rng(seed)
    normal = rng.integers(0, 256, 3 * total, dtype=np.uint8)
    normal[np.repeat(rng.random(total) < 0.4, 3)] = 128
    if kind == "constant":
        return np.full(total, 7, np.uint16), np.full(total, 0, np.uint16), normal
    if kind == "runs":
        which = np.repeat(np.arange(total) % 2, rng.integers(1, 700, total))[:total].astype(bool)
        return np.where(which, 300, 12).astype(np.uint16), np.where(which, 0, 100).astype(np.uint16), normal
    small = rng.random(total) < 0.5
    sdf = np.where(small, rng.integers(0, 300, total), rng.integers(0, 65536, total)).astype(np.uint16)
    iters = np.where(~small, rng.integers(0, 101, total), rng.integers(0, 65536, total)).astype(np.uint16)
    for i, v in enumerate(EXTREMES[:total]):
        sdf[i], iters[i] = v, EXTREMES[len(EXTREMES) - 1 - i]
    return sdf, iters, normal


def to_dev(x, shift=0):
    """A CUDA tensor with x's bytes; shift: the tensor starts one element past its allocation."""
    import torch
    if x is None:
        return None
    t = torch.empty(x.size + 1, dtype=torch.int16 if x.dtype == np.uint16 else torch.uint8, device="cuda:0")
    view = t[1:] if shift else t[:-1]
    view.copy_(torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x))
    return view


class Out:
    """Image and record buffers pre-filled with 0xFF, a guard region behind each."""

    def __init__(self, total, n, shift=0):
        import torch
        self.total, self.n = total, n
        self._rgba = torch.full((4 * (total + GUARD) + 4,), 0xFF, dtype=torch.uint8, device="cuda:0")
        self.rgba = self._rgba[shift:shift + 4 * (total + GUARD)]  # shift 1: one element (a byte) past the allocation
        self.hist = torch.full((REC * (n + GUARD),), 0xFF, dtype=torch.uint8, device="cuda:0")

    def check_hist(self, ctx, want, what):
        import torch
        torch.cuda.synchronize()
        raw = self.hist.cpu().numpy()
        got = ctx.decode_hists(raw[:REC * self.n])
        assert len(got) == len(want) == self.n
        for k in range(self.n):
            for name in ("sdf", "iters"):
                bad = M.same(got[k][name], want[k][name])
                assert not bad, "%s: frame %d %s: %s" % (what, k, name, bad)
        assert (raw[REC * self.n:] == 0xFF).all(), what + ": records written past the last frame"
        return got

    def check_image(self, want, what):
        import torch
        torch.cuda.synchronize()
        rgba = self.rgba.cpu().numpy()
        if want is None:
            assert (rgba == 0xFF).all(), what + ": image written"
            return
        bad = int((rgba[:4 * self.total] != want).sum())
        assert bad == 0, "%s: %d image bytes differ" % (what, bad)
        assert (rgba[4 * self.total:] == 0xFF).all(), what + ": image written past the last frame"


def run_hist(ctx, data, W, rows, n, mask="all", shift=0, permille=(0, 1000), past=0, sdf=True, iters=True, what=""):
    """One device call on buffers of their own against the model; returns the decoded records."""
    s, i, nrm = data
    s, i = (s if sdf else None), (i if iters else None)
    out = Out(W * rows * n, n)
    ctx.counter_hist(to_dev(s, past), to_dev(i, past), normal=to_dev(nrm, past) if mask != "all" or past else None, mask=mask,
                     bin_shift=shift, percentiles=permille, hist=out.hist, width=W, rows=rows, n_frames=n)
    assert ctx.last_kernel() == ("hist_kernel<false>" if mask == "all" else "hist_kernel<true>")
    want = M.counter_hist(s, i, nrm, W * rows, n, M.MASKS[mask], shift, *permille)
    return out.check_hist(ctx, want, what or "%dx%dx%d %s shift %d %s" % (W, rows, n, mask, shift, permille))


def run_shade(ctx, values, W, rows, n, lo, hi, counter="sdf", past=0, what=""):
    out = Out(W * rows * n, n, shift=past)
    ctx.shade_ranged(counter, to_dev(values, past), out.rgba, lo=lo, hi=hi, width=W, rows=rows, n_frames=n)
    if W * rows * n:
        assert ctx.last_kernel() == "shade_ranged_kernel"
    out.check_image(M.shade_ranged(values, W * rows, n, [(lo, hi)] * n) if W * rows * n else None,
                    what or "shade %dx%dx%d [%d, %d]" % (W, rows, n, lo, hi))
    return out


@pytest.fixture(scope="module")
def hctx(rm):
    ctx = rm.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def big():
    """Two frames of 256 x 129 of each kind, made once."""
    return {kind: synth(40 + k, 2 * 256 * 129, kind) for k, kind in enumerate(("random", "constant", "runs"))}


# ---------------------------------------------------------------------------------------- GPU, synthetic buffers

COUNTS = [0, 1, 15, 16, 17, 31, 47, 4096, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("npx", COUNTS)
def test_pixel_counts_around_the_group_and_the_workgroup(rm, hctx, npx):
    """Head and tail paths (below and around the 16-pixel group), the one-workgroup path (4 096) and the first frame of two
    workgroups (4 097), one and two frames, every mask; the ranged shade on the same shapes with lo == hi, lo = 0, hi = 65535."""
    for n in (1, 2):
        data = synth(npx * 10 + n, max(npx * n, 16))  # (a tensor without elements has no address to pass)
        for k, mask in enumerate(("all", "surface", "background")):
            run_hist(hctx, data, npx, 1, n, mask, (0, 3, 8)[k], PERMILLES[k])
        for lo, hi in ((0, 65535), (255, 255), (0, 51), (3, 300), (0, 0), (65535, 65535)):
            run_shade(hctx, data[0], npx, 1, n, lo, hi)
        run_shade(hctx, data[1], npx, 1, n, 10, 100000, counter="iters", past=1)


@pytest.mark.gpu
def test_three_frames_each_aligned_differently(rm, hctx):
    """Three frames of 33 x 7 (231 pixels: every frame's slices start off another alignment) in buffers that start one element
    past their allocation: every mask with both counters, then each counter absent in turn."""
    W, rows, n = 33, 7, 3
    data = synth(5, W * rows * n)
    for mask in ("all", "surface", "background"):
        for past in (0, 1):
            run_hist(hctx, data, W, rows, n, mask, 0, (10, 990), past=past)
            got = run_hist(hctx, data, W, rows, n, mask, 3, (500, 500), past=past, sdf=False)
            assert all(not M.same(g["sdf"], M.zero(3)) for g in got)
            got = run_hist(hctx, data, W, rows, n, mask, 8, (0, 1000), past=past, iters=False)
            assert all(not M.same(g["iters"], M.zero(8)) for g in got)
    for past in (0, 1):
        run_shade(hctx, data[0], W, rows, n, 2, 40000, past=past)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "constant", "runs"])
def test_frames_of_several_workgroups(rm, hctx, big, kind):
    """Two frames of 256 x 129 (9 workgroups each: the cross-workgroup combine): seeded random values with the extremes in the
    first pixels, a constant frame (every lane of every wave in one bin) and two values in runs; shifts 0, 3 and 8, the three
    permille pairs, all three masks."""
    W, rows, n = 256, 129, 2
    for k, shift in enumerate((0, 3, 8)):
        for j, permille in enumerate(PERMILLES):
            run_hist(hctx, big[kind], W, rows, n, ("all", "surface", "background")[(k + j) % 3], shift, permille)
    got = run_hist(hctx, big[kind], W, rows, n, "all", 0, (0, 1000))
    for g in got:
        assert int(g["sdf"]["bins"].sum()) == g["sdf"]["pixels"] == W * rows
    run_shade(hctx, big[kind][0], W, rows, n, 5, 290)


@pytest.mark.gpu
def test_calls_in_flight_share_the_ring(rm, big):
    """Two calls of 2 x 256 x 129 on two streams without a synchronisation between them, then a third on the first stream, on a
    context of their own: all three equal the model, so no call met another's scratch entries and each left them zeroed."""
    import torch
    W, rows, n = 256, 129, 2
    s, i, nrm = big["random"]
    ds, di, dn = to_dev(s), to_dev(i), to_dev(nrm)
    ctx = rm.Context(0)
    streams = [torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")]
    outs = [Out(0, n) for _ in range(3)]
    masks = ("all", "surface", "all")
    torch.cuda.synchronize()  # (the 0xFF fills and the copies ran on the default stream)
    for k in range(3):
        with torch.cuda.stream(streams[k % 2]):
            ctx.counter_hist(ds, di, normal=dn, mask=masks[k], bin_shift=0, percentiles=(10, 990), hist=outs[k].hist, width=W, rows=rows,
                             n_frames=n)
    for k in range(3):
        outs[k].check_hist(ctx, M.counter_hist(s, i, nrm, W * rows, n, M.MASKS[masks[k]], 0, 10, 990), "call %d" % k)
    ctx.close()


@pytest.mark.gpu
def test_no_pixel_and_no_frame(rm, hctx):
    data = synth(3, 64)
    for W, rows in ((0, 7), (7, 0), (0, 0)):
        got = run_hist(hctx, data, W, rows, 3, "surface", 4, (10, 990))
        assert all(not M.same(g[c], M.zero(4)) for g in got for c in ("sdf", "iters"))
        run_shade(hctx, data[0], W, rows, 3, 0, 9)
    out = Out(0, 0)
    hctx.counter_hist(to_dev(data[0]), to_dev(data[1]), hist=out.hist, width=8, rows=8, n_frames=0)
    out.check_hist(hctx, [], "no frame")
    hctx.shade_ranged("sdf", to_dev(data[0]), out.rgba, lo=0, hi=9, width=8, rows=8, n_frames=0)
    out.check_image(None, "no frame")


@pytest.mark.gpu
def test_shade_from_records_written_in_the_same_stream(rm, hctx, big):
    """counter_hist, then shade_ranged of each counter from its records, with no synchronisation in between: each frame is scaled
    to its own range.  The frames differ in range (the second frame's values are halved)."""
    W, rows, n = 256, 129, 2
    s, i, nrm = (x.copy() for x in big["random"])
    s[W * rows:] //= 2
    i[W * rows:] //= 3
    ds, di, dn = to_dev(s, 1), to_dev(i, 1), to_dev(nrm, 1)
    want = M.counter_hist(s, i, nrm, W * rows, n, M.MASKS["surface"], 0, 10, 990)
    assert want[0]["sdf"]["range_hi"] != want[1]["sdf"]["range_hi"]
    for counter, dv, v in (("sdf", ds, s), ("iters", di, i)):
        out = Out(W * rows * n, n, shift=1)
        hctx.counter_hist(ds, di, normal=dn, mask="surface", percentiles=(10, 990), hist=out.hist, width=W, rows=rows, n_frames=n)
        hctx.shade_ranged(counter, dv, out.rgba, hist=out.hist, lo=9, hi=3, width=W, rows=rows, n_frames=n)  # (lo, hi: ignored)
        out.check_hist(hctx, want, "records")
        out.check_image(M.shade_ranged(v, W * rows, n, [(w[counter]["range_lo"], w[counter]["range_hi"]) for w in want]), "from records, " + counter)


@pytest.mark.gpu
def test_range_0_to_51_is_the_reference_heatmap(rm, hctx):
    """lo = 0, hi = 51 on values <= 51: s = v * 255 // 51 = 5 v = v * 5 % 256 -- the image of rm_shade_device's two heatmaps."""
    import torch
    W, rows = 65, 31
    rng = np.random.default_rng(8)
    s, i = rng.integers(0, 52, W * rows).astype(np.uint16), rng.integers(0, 52, W * rows).astype(np.uint16)
    s[:3], i[:3] = (0, 51, 50), (51, 0, 1)
    depth, nrm = torch.zeros(W * rows, dtype=torch.uint8, device="cuda:0"), torch.zeros(3 * W * rows, dtype=torch.uint8, device="cuda:0")
    ds, di = to_dev(s), to_dev(i)
    for counter, dv, shader in (("sdf", ds, 2), ("iters", di, 3)):
        ref = torch.empty(4 * W * rows, dtype=torch.uint8, device="cuda:0")
        hctx.shade(shader, W, rows, depth, nrm, ds, di, ref)
        out = Out(W * rows, 1)
        hctx.shade_ranged(counter, dv, out.rgba, lo=0, hi=51, width=W, rows=rows)
        out.check_image(ref.cpu().numpy(), "against rm_shade_device, " + counter)


@pytest.mark.gpu
def test_host_entries_equal_device_entries(rm, hctx):
    W, rows, n = 65, 7, 3
    s, i, nrm = synth(11, W * rows * n)
    dev = Out(W * rows * n, n)
    hctx.counter_hist(to_dev(s), to_dev(i), normal=to_dev(nrm), mask="background", bin_shift=2, percentiles=(250, 750), hist=dev.hist, width=W,
                      rows=rows, n_frames=n)
    hctx.shade_ranged("iters", to_dev(i), dev.rgba, hist=dev.hist, width=W, rows=rows, n_frames=n)
    import torch
    torch.cuda.synchronize()
    hist = np.full(REC * (n + 1), 0xFF, np.uint8)
    hctx.counter_hist(s, i, normal=nrm, mask="background", bin_shift=2, percentiles=(250, 750), hist=hist, width=W, rows=rows, n_frames=n)
    assert np.array_equal(hist[:REC * n], dev.hist.cpu().numpy()[:REC * n]) and (hist[REC * n:] == 0xFF).all()
    rgba = np.full(4 * W * rows * n + 16, 0xFF, np.uint8)
    hctx.shade_ranged("iters", i, rgba, hist=hist[:REC * n], width=W, rows=rows, n_frames=n)
    assert np.array_equal(rgba[:-16], dev.rgba.cpu().numpy()[:4 * W * rows * n]) and (rgba[-16:] == 0xFF).all()
    rgba2 = np.full(4 * W * rows * n, 0xFF, np.uint8)
    hctx.shade_ranged("sdf", s, rgba2, lo=3, hi=400, width=W, rows=rows, n_frames=n)
    assert np.array_equal(rgba2, M.shade_ranged(s, W * rows, n, [(3, 400)] * n))
    allocated = hctx.counter_hist(s, None, width=W, rows=rows, n_frames=n)  # hist=None: a numpy buffer beside numpy counters
    got = hctx.decode_hists(allocated)
    want = M.counter_hist(s, None, None, W * rows, n, 0, 0, 0, 1000)
    assert all(not M.same(g[c], w[c]) for g, w in zip(got, want) for c in ("sdf", "iters"))
    empty = np.full(REC * 2, 0xFF, np.uint8)
    hctx.counter_hist(s, i, bin_shift=5, hist=empty, width=0, rows=4, n_frames=2)
    assert all(not M.same(g[c], M.zero(5)) for g in hctx.decode_hists(empty) for c in ("sdf", "iters"))


# ---------------------------------------------------------------------------------------- GPU, rendered


def make_job(N, W, H, preset, accel):
    j = N.rm_job()
    j.width, j.height, j.y_start, j.y_end = W, H, 0, H
    j.algorithm = N.lib().rm_algorithm_from_string(b"sphere-tracer")
    j.scene_preset_index, j.acceleration_structure = preset, {"None": 0, "Octree": 1, "BVH": 2}[accel]
    j.overshoot_factor, j.step_size = float("nan"), float("nan")
    return j


@pytest.fixture(scope="module")
def rendered(rm):
    """Preset 3 with the BVH, a 4-view yaw sweep at 64 x 64 through render_frames with its per-frame accumulators, rendered once."""
    import torch
    from cpu_raymarcher_amd import _native as N
    W = H = 64
    n, total = 4, 4 * 64 * 64
    ctx = rm.Context(0)
    g = (torch.empty(total, dtype=torch.uint8, device="cuda:0"), torch.empty(3 * total, dtype=torch.uint8, device="cuda:0"),
         torch.empty(total, dtype=torch.int16, device="cuda:0"), torch.empty(total, dtype=torch.int16, device="cuda:0"))
    acc = torch.empty(4 * n, dtype=torch.int64, device="cuda:0")
    ctx.render_frames(make_job(N, W, H, 3, "BVH"), rm.sweep_views(0.1, 0.0, 0.0, 0.4, n=n), *g, diag=acc)
    torch.cuda.synchronize()
    yield ctx, W, H, n, g, ctx.decode_accs(acc)
    ctx.close()


@pytest.mark.gpu
def test_rendered_sweep_against_its_accumulators(rm, rendered):
    ctx, W, H, n, g, accs = rendered
    host = [x.cpu().numpy().view(np.uint16) if x.element_size() == 2 else x.cpu().numpy() for x in g]
    recs = {}
    for mask in ("all", "surface", "background"):
        out = Out(0, n)
        ctx.counter_hist(g[2], g[3], normal=g[1], mask=mask, percentiles=(500, 990), hist=out.hist, width=W, rows=H, n_frames=n)
        recs[mask] = out.check_hist(ctx, M.counter_hist(host[2], host[3], host[1], W * H, n, M.MASKS[mask], 0, 500, 990), "rendered, " + mask)
    for k in range(n):
        a, s, b = (recs[m][k] for m in ("all", "surface", "background"))
        assert (a["sdf"]["sum"], a["iters"]["sum"], a["sdf"]["min"], a["sdf"]["max"]) == \
            (accs[k]["total_sdf"], accs[k]["total_iters"], accs[k]["min_sdf"], accs[k]["max_sdf"])
        for c in ("sdf", "iters"):
            assert a[c]["pixels"] == W * H == int(a[c]["bins"].sum())
            assert s[c]["pixels"] > 0 and b[c]["pixels"] > 0
            assert a[c]["pixels"] == s[c]["pixels"] + b[c]["pixels"] and a[c]["sum"] == s[c]["sum"] + b[c]["sum"]
            assert a[c]["min"] == min(s[c]["min"], b[c]["min"]) and a[c]["max"] == max(s[c]["max"], b[c]["max"])
            assert np.array_equal(a[c]["bins"], s[c]["bins"] + b[c]["bins"])
            assert rm.percentile(s[c], 500)[0] == s[c]["range_lo"] and rm.percentile(s[c], 990)[1] == s[c]["range_hi"]


@pytest.mark.gpu
def test_ranged_heatmap_models_equal_the_calls_they_wrap(rm, rendered):
    """RangedSDFHeatmap / RangedIterationHeatmap.shade on the first rendered frame, device and host buffers: the bytes of
    counter_hist with percentiles (0, hi_permille) of the model's own counter followed by shade_ranged from that record."""
    import torch
    ctx, W, H, n, g, accs = rendered
    npx = W * H
    frame = [x[:npx * e].contiguous() for x, e in zip(g, (1, 3, 1, 1))]
    for cls, counter, values in ((rm.RangedSDFHeatmap, "sdf", frame[2]), (rm.RangedIterationHeatmap, "iters", frame[3])):
        for mask, permille in (("all", 1000), ("surface", 990)):
            model = cls(ctx, hi_permille=permille, mask=mask)
            shaded = torch.full((4 * npx,), 0xFF, dtype=torch.uint8, device="cuda:0")
            assert model.shade(shaded, *frame, W, H) is shaded
            out = Out(npx, 1)
            ctx.counter_hist(values if counter == "sdf" else None, values if counter == "iters" else None, normal=frame[1], mask=mask,
                             percentiles=(0, permille), hist=out.hist, width=W, rows=H)
            ctx.shade_ranged(counter, values, out.rgba, hist=out.hist, width=W, rows=H)
            out.check_image(shaded.cpu().numpy(), "%s %s" % (cls.__name__, mask))
            assert np.array_equal(model.hist.cpu().numpy(), out.hist.cpu().numpy()[:REC])
            host = [x.cpu().numpy().view(np.uint16) if x.element_size() == 2 else x.cpu().numpy() for x in frame]
            on_host = np.full(4 * npx, 0xFF, np.uint8)
            cls(ctx, hi_permille=permille, mask=mask).shade(on_host, *host, W, H)
            assert np.array_equal(on_host, shaded.cpu().numpy())
    assert type(rm.createShadingModelFromValue("ranged-sdf-heatmap", ctx)).__name__ == "NormalModel"  # the factory is the reference's


# ---------------------------------------------------------------------------------------- CPU


def test_model_on_cases_worked_by_hand():
    # five values, sorted 1 1 3 4 5: rank floor(500 * 4 / 1000) = 2 is 3, rank floor(990 * 4 / 1000) = 3 is 4
    r = M.counter_record(np.array([3, 1, 4, 1, 5], np.uint16), 0, 500, 990)
    assert {f: r[f] for f in M.FIELDS} == dict(pixels=5, sum=14, min=1, max=5, range_lo=3, range_hi=4, shift=0, reserved=0)
    assert r["bins"][:6].tolist() == [0, 2, 0, 1, 1, 1] and int(r["bins"].sum()) == 5
    r = M.counter_record(np.array([3, 1, 4, 1, 5], np.uint16), 0, 0, 1000)
    assert (r["range_lo"], r["range_hi"]) == (1, 5)
    # shift 0: 255, 256 and 65535 share the last bin, whose upper end is the maximum
    v = np.array([254, 255, 256, 65535], np.uint16)
    r = M.counter_record(v, 0, 0, 1000)
    assert r["bins"][254] == 1 and r["bins"][255] == 3 and (r["range_lo"], r["range_hi"]) == (254, 65535)
    r = M.counter_record(v, 0, 500, 500)  # rank 1: bin 255
    assert (r["range_lo"], r["range_hi"]) == (255, 65535)
    # shift 8: bins of 256 values; 254 and 255 in bin 0, 256 in bin 1, 65535 in bin 255
    r = M.counter_record(v, 8, 0, 500)
    assert r["bins"][0] == 2 and r["bins"][1] == 1 and r["bins"][255] == 1 and r["shift"] == 8
    assert (r["range_lo"], r["range_hi"]) == (254, 255)  # max(min, 0 << 8), min(max, (1 << 8) - 1)
    r = M.counter_record(v, 8, 750, 1000)  # rank 2: bin 1; rank 3: bin 255
    assert (r["range_lo"], r["range_hi"]) == (256, 65535)
    # no pixel
    r = M.counter_record(np.zeros(0, np.uint16), 3, 10, 990)
    assert not M.same(r, M.zero(3)) and r["shift"] == 3
    nrm = np.full(6, 128, np.uint8)
    got = M.counter_hist(np.array([7, 9], np.uint16), None, nrm, 2, 1, M.MASKS["surface"], 0, 0, 1000)
    assert not M.same(got[0]["sdf"], M.zero(0)) and not M.same(got[0]["iters"], M.zero(0))
    # the ramp: s = 0 up to lo, 255 from hi, integer division between
    img = M.shade_ranged(np.array([0, 10, 11, 60, 110, 200], np.uint16), 6, 1, [(10, 110)]).reshape(-1, 4)
    assert img.tolist() == [[0, 255, 0, 255], [0, 255, 0, 255], [4, 255, 0, 255], [254, 255, 0, 255], [255, 2, 0, 255], [255, 2, 0, 255]]


def test_range_lo_never_exceeds_range_hi():
    from cpu_raymarcher_amd.context import percentile
    rng = np.random.default_rng(1)
    for trial in range(300):
        n = int(rng.integers(1, 200))
        v = rng.integers(0, (300, 65536)[trial % 2], n).astype(np.uint16)
        shift = int(rng.integers(0, 9))
        lo = int(rng.integers(0, 1001))
        hi = int(rng.integers(lo, 1001))
        r = M.counter_record(v, shift, lo, hi)
        assert r["min"] <= r["range_lo"] <= r["range_hi"] <= r["max"], (v, shift, lo, hi, r)
        assert percentile(r, lo)[0] == r["range_lo"] and percentile(r, hi)[1] == r["range_hi"]
        if shift == 0 and r["max"] < 255:  # the exact nearest-rank percentiles
            srt = np.sort(v)
            assert (r["range_lo"], r["range_hi"]) == (srt[lo * (n - 1) // 1000], srt[hi * (n - 1) // 1000])


def test_struct_layout(rm):
    from cpu_raymarcher_amd import _native as N
    assert C.sizeof(N.rm_counter_hist) == 1064 and C.sizeof(N.rm_frame_hist) == REC == 2128
    assert N.rm_counter_hist.bins.offset == 40 and N.rm_frame_hist.iters.offset == 1064
    assert tuple(f for f, _ in N.rm_counter_hist._fields_) == M.FIELDS + ("bins",)


def test_host_only_context_checks_arguments_first(rm):
    """Every refusal of the header on a context without a device, device and host entry alike: the checks come before the device
    check.  Valid arguments: RM_E_NO_DEVICE, also for frames without a pixel."""
    from cpu_raymarcher_amd import _native as N
    L = N.lib()
    ctx = rm.Context(None)
    buf = np.zeros(8192, np.uint16)
    p = buf.ctypes.data
    BIG = 65536  # 65536 x 65536 pixels > UINT32_MAX

    def hist(width=8, rows=8, n=1, sdf=p, iters=p, normal=p, mask=0, shift=0, lo=0, hi=1000, out=p):
        d = L.rm_counter_hist_device(ctx._h, width, rows, n, sdf, iters, normal, mask, shift, lo, hi, out, None)
        h = L.rm_counter_hist(ctx._h, width, rows, n, sdf, iters, normal, mask, shift, lo, hi, out)
        assert d == h, (d, h)
        return d

    def shade(counter=0, width=8, rows=8, n=1, values=p, rec=None, lo=0, hi=10, rgba=p):
        d = L.rm_shade_ranged_device(ctx._h, counter, width, rows, n, values, rec, lo, hi, rgba, None)
        h = L.rm_shade_ranged(ctx._h, counter, width, rows, n, values, rec, lo, hi, rgba)
        assert d == h, (d, h)
        return d

    for ok in (dict(), dict(width=0), dict(n=0), dict(n=65535), dict(normal=None), dict(sdf=None), dict(iters=None), dict(mask=2), dict(shift=8),
               dict(lo=500, hi=500), dict(lo=1000, hi=1000), dict(width=65535, rows=65537)):
        assert hist(**ok) == N.RM_E_NO_DEVICE, ok
    for bad in (dict(out=None), dict(sdf=None, iters=None), dict(width=-1), dict(rows=-1), dict(n=-1), dict(width=BIG, rows=BIG), dict(n=65536),
                dict(mask=-1), dict(mask=3), dict(mask=1, normal=None), dict(mask=2, normal=None), dict(shift=-1), dict(shift=9),
                dict(lo=-1), dict(hi=1001), dict(lo=600, hi=599), dict(sdf=p + 1), dict(iters=p + 1), dict(out=p + 4)):
        assert hist(**bad) == N.RM_E_INVALID, bad
        assert L.rm_last_error(ctx._h)
    for ok in (dict(), dict(counter=1), dict(width=0), dict(n=0), dict(lo=7, hi=7), dict(rec=p, lo=9, hi=3), dict(lo=0, hi=2 ** 32 - 1)):
        assert shade(**ok) == N.RM_E_NO_DEVICE, ok
    for bad in (dict(rgba=None), dict(values=None), dict(counter=2), dict(counter=-1), dict(width=-1), dict(rows=-1), dict(n=-1),
                dict(width=BIG, rows=BIG), dict(n=65536), dict(lo=4, hi=3), dict(values=p + 1), dict(rec=p + 4)):
        assert shade(**bad) == N.RM_E_INVALID, bad
    assert L.rm_counter_hist_device(None, 8, 8, 1, p, p, p, 0, 0, 0, 1000, p, None) == N.RM_E_INVALID
    assert L.rm_shade_ranged_device(None, 0, 8, 8, 1, p, None, 0, 1, p, None) == N.RM_E_INVALID
    with pytest.raises(N.RmError) as e:
        ctx.counter_hist(np.zeros(64, np.uint16), None, width=8, rows=8)
    assert e.value.code == N.RM_E_NO_DEVICE
    ctx.close()


def test_new_kernels_spill_no_vgpr_and_use_no_scratch():
    """hist_kernel<false>, hist_kernel<true> and shade_ranged_kernel on the compiler's own resource-usage listing."""
    import test_build_invariants as B
    if not B.os.path.exists(B.HIPCC) or B.shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = B.resource_usage((), "rm_frame_ops.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith(("void hist_kernel<", "shade_ranged_kernel("))}
    assert len(kernels) == 3, sorted(usage)
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
