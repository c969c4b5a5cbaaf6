"""Option `min_fill`: a persistent launch of the v2 wave loop brings at least ceil(6 / Q) workgroups per CU, Q being the
hardware queues of the process (GPU_MAX_HW_QUEUES as rm_create found it; HIP's default 4).  Launches on streams that share a
queue run one after the other, so no launch overlaps with more than Q - 1 others, and a CU holds six of the kernel's workgroups.

Host part (no GPU): how the variable is read, that a context keeps what it read, the rule itself through
rm_debug_launch_fill, the option's switch contract, and that `blocks_per_cu` reads back as set.  GPU part: the grid the
launcher really uses (rm_debug_last_launch) and that the bytes do not depend on it."""
import hashlib
import io
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "GPU_MAX_HW_QUEUES"
WAVES = 6  # RM_V2_WAVES: four-wave workgroups of the wave loop a CU holds


def rule(asked, queues, min_fill):
    return max(asked, -(-WAVES // queues)) if min_fill else asked


def host_ctx(rm, monkeypatch, value):
    if value is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, value)
    return rm.Context(None)


@pytest.mark.parametrize("value, queues", [(None, 4), ("", 4), ("abc", 4), ("0", 4), ("-3", 4), ("1", 1), ("4", 4), ("16", 16), ("64", 64)])
def test_queue_count_is_read_from_the_environment(rm, monkeypatch, value, queues):
    """Unset, empty, not a number or <= 0 mean HIP's default of four; a decimal integer >= 1 is taken as it is.  Seen through
    the rule: with Q queues a request of one workgroup per CU becomes ceil(6 / Q)."""
    ctx = host_ctx(rm, monkeypatch, value)
    assert ctx.launch_fill(1) == -(-WAVES // queues)
    assert os.environ.get(ENV) == value  # read, never set
    ctx.close()


def test_a_context_keeps_the_count_it_read(rm, monkeypatch):
    a = host_ctx(rm, monkeypatch, "2")
    assert a.launch_fill(1) == 3
    monkeypatch.setenv(ENV, "16")
    b = rm.Context(None)
    assert (a.launch_fill(1), b.launch_fill(1)) == (3, 1)
    monkeypatch.delenv(ENV)
    assert (a.launch_fill(1), b.launch_fill(1), rm.Context(None).launch_fill(1)) == (3, 1, 2)
    a.close()
    b.close()


@pytest.mark.parametrize("queues", [1, 2, 3, 4, 5, 6, 16])
def test_the_rule(rm, monkeypatch, queues):
    """max(asked, ceil(6 / Q)) with `min_fill` on, `asked` with it off; Q = 1, 2, 3, 4 give floors of 6, 3, 2, 2, Q >= 6 gives
    1: such processes launch exactly as before.  `blocks_per_cu` reads back as it was set whatever the launcher makes of it."""
    ctx = host_ctx(rm, monkeypatch, str(queues))
    assert ctx.get_option("min_fill") == 1
    assert rule(1, queues, 1) == {1: 6, 2: 3, 3: 2, 4: 2, 5: 2, 6: 1, 16: 1}[queues]
    for min_fill in (1, 0, 1):
        ctx.set_option("min_fill", min_fill)
        for asked in range(1, 9):
            assert ctx.launch_fill(asked) == rule(asked, queues, min_fill), (queues, asked, min_fill)
            ctx.set_option("blocks_per_cu", asked)
            assert ctx.get_option("blocks_per_cu") == asked
    for bad in (0, 9, -1):
        with pytest.raises(rm.RmError):
            ctx.launch_fill(bad)
    ctx.close()


def test_min_fill_keeps_the_switch_contract(rm):
    """As tests/test_host_logic.py test_every_option_keeps_its_contract has it for a 0 | 1 switch: default, any non-zero value
    is 1, nothing is refused, and no other key's value moves."""
    ctx = rm.Context(None)
    others = ("blocks_per_cu", "lds_fill", "lds_kb", "item_px", "refill", "lpt")
    before = {k: ctx.get_option(k) for k in others}
    assert ctx.get_option("min_fill") == 1
    for probe, stored in [(0, 0), (1, 1), (7, 1), (-1, 1), (0, 0), (1 << 40, 1), (-(1 << 40), 1)]:
        ctx.set_option("min_fill", probe)
        assert ctx.get_option("min_fill") == stored, probe
        assert {k: ctx.get_option(k) for k in others} == before
    for k in others:  # ... and no other key writes this one
        ctx.set_option(k, before[k])
        assert ctx.get_option("min_fill") == 1
    ctx.close()


def test_last_launch_of_a_host_only_context(rm):
    ctx = rm.Context(None)
    assert ctx.last_launch() == dict(workgroups=0, threads=0, lds_bytes=0, cus=256)
    ctx.close()


def test_trace_overlap_on_a_made_up_trace(tmp_path):
    """scripts/trace_overlap.py: two launches of 256 workgroups overlap for half of the time one of them runs, a launch of 512
    runs alone afterwards; other kernels are left out."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import trace_overlap as T
    finally:
        sys.path.pop(0)
    cols = ["Kind", "Queue_Id", "Kernel_Name", "Start_Timestamp", "End_Timestamp", "Workgroup_Size_X", "Workgroup_Size_Y",
            "Workgroup_Size_Z", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"]
    rows = [("KERNEL_DISPATCH", 1, "rm_rtc_render_v2", 1000, 3000, 256, 1, 1, 256 * 256, 1, 1),
            ("KERNEL_DISPATCH", 2, "void render_kernel_v2<2, true, true, false>(RmRenderParams)", 2000, 4000, 256, 1, 1, 256 * 256, 1, 1),
            ("KERNEL_DISPATCH", 1, "__amd_rocclr_fillBufferAligned", 0, 10000, 256, 1, 1, 65536, 1, 1),
            ("KERNEL_DISPATCH", 1, "rm_rtc_render_v2", 5000, 6000, 256, 1, 1, 512 * 256, 1, 1)]
    path = tmp_path / "t_kernel_trace.csv"
    path.write_text(",".join('"%s"' % c for c in cols) + "\n" + "\n".join(",".join('"%s"' % v if isinstance(v, str) else str(v) for v in r) for r in rows) + "\n")
    k = T.read_kernels(str(path), T.DEFAULT_MATCH)
    assert [(a, b, g, w) for a, b, g, w, _, _ in k] == [(1000, 3000, 256, 256), (2000, 4000, 256, 256), (5000, 6000, 512, 256)]
    span, at_once, per_cu = T.weighted(k, 256)
    assert span == 5000 and at_once == {1: 3000, 2: 1000, 0: 1000} and per_cu == {1.0: 2000, 2.0: 2000, 0.0: 1000}
    out = io.StringIO()
    T.report(k, 256, out=out)
    assert "mean 1.25, most 2" in out.getvalue() and "mean asked 1.50" in out.getvalue()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------

W, H = 640, 360  # item_px 64 with 8-pixel wave rows: 80 x 45 = 3 600 items, 900 workgroups of four waves: more than 3 x 256 CUs
NEEDED = (W // 8) * (H // 8) // 4


def gpu_scene(rm, monkeypatch, queues, **opts):
    monkeypatch.setenv(ENV, str(queues))  # what the library reads; the HIP runtime of this process started long ago
    ctx = rm.Context(0)
    for k, v in dict(blocks_per_cu=1, item_px=64, tile_w=8, **opts).items():
        ctx.set_option(k, v)
    scene = rm.Scene("BVH", ctx=ctx)
    scene.loadPreset(3)
    return ctx, scene


def render(rm, ctx, scene, w=W, h=H, stream=None):
    """One frame with the fused shade and the fused diagnostics -> (SHA-256 of the five buffers and the diagnostics, last launch)."""
    import torch
    dev = torch.device("cuda:0")
    with torch.cuda.stream(stream or torch.cuda.current_stream(dev)):
        b = dict(depth=torch.zeros(w * h, dtype=torch.uint8, device=dev), normal=torch.zeros(3 * w * h, dtype=torch.uint8, device=dev),
                 sdf=torch.zeros(w * h, dtype=torch.int16, device=dev), iters=torch.zeros(w * h, dtype=torch.int16, device=dev),
                 rgba=torch.zeros(4 * w * h, dtype=torch.uint8, device=dev), acc=torch.full((4,), -1, dtype=torch.int64, device=dev))
        rm.SphereTracer().runRaymarcher(scene, b["depth"], b["normal"], b["sdf"], b["iters"], w, h, 0.0, shadedBuffer=b["rgba"],
                                        shader="iteration-heatmap", diagnostics=b["acc"])
    return b, ctx.last_launch()


def digest(b):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(b"".join(b[k].cpu().numpy().tobytes() for k in ("depth", "normal", "sdf", "iters", "rgba", "acc"))).hexdigest()


@pytest.mark.gpu
def test_four_queues_bring_two_workgroups_per_cu(rm, monkeypatch):
    """Q = 4, one workgroup per CU asked: `min_fill` 1 launches 2 x CUs workgroups, 0 launches 1 x CUs; the five buffers and the
    fused diagnostics are the same bytes, and those of the one-ray-per-lane kernel.  Three asked are three either way; a frame
    of 16 workgroups launches 16; `lds_fill` goes by what was asked (1: never pad), not by what the launch brings."""
    ctx, scene = gpu_scene(rm, monkeypatch, 4, specialise_v2_after=0)
    cus = ctx.last_launch()["cus"]
    assert NEEDED == 900 and NEEDED > 3 * cus, "the frame must need more workgroups than any launch here brings"
    got = {}
    for min_fill in (1, 0):
        ctx.set_option("min_fill", min_fill)
        b, shape = render(rm, ctx, scene)
        assert "render_kernel_v2<2, true, true, false>" in ctx.last_kernel()
        assert (shape["workgroups"], shape["threads"]) == ((2 if min_fill else 1) * cus, 256), (min_fill, shape)
        got[min_fill] = (digest(b), shape["lds_bytes"])
        assert ctx.get_option("blocks_per_cu") == 1
    assert got[1] == got[0]  # bytes and LDS request
    ctx.set_option("kernel", 1)
    b, _ = render(rm, ctx, scene)
    assert "render_kernel_v2" not in ctx.last_kernel() and digest(b) == got[1][0]
    ctx.set_option("kernel", 0)
    for min_fill in (1, 0):
        ctx.set_option("min_fill", min_fill)
        ctx.set_option("blocks_per_cu", 3)
        b, shape = render(rm, ctx, scene)
        assert shape["workgroups"] == 3 * cus and digest(b) == got[1][0], (min_fill, shape)
        ctx.set_option("blocks_per_cu", 1)
        _, shape = render(rm, ctx, scene, 64, 64)
        assert shape["workgroups"] == 16, (min_fill, shape)
        ctx.set_option("lds_fill", 1)  # asked 1: no padding, although the launch brings two with min_fill on
        b, shape = render(rm, ctx, scene)
        assert (shape["workgroups"], shape["lds_bytes"]) == ((2 if min_fill else 1) * cus, got[1][1]) and digest(b) == got[1][0], (min_fill, shape)
        ctx.set_option("blocks_per_cu", 3)  # asked 3: padded so that exactly three fit, as before
        _, padded = render(rm, ctx, scene)
        assert padded["workgroups"] == 3 * cus and padded["lds_bytes"] > got[1][1], (min_fill, padded)
        ctx.set_option("lds_fill", 0)
        ctx.set_option("blocks_per_cu", 1)
    ctx.close()


@pytest.mark.gpu
def test_sixteen_queues_launch_as_asked(rm, monkeypatch):
    ctx, scene = gpu_scene(rm, monkeypatch, 16, specialise_v2_after=0)
    cus = ctx.last_launch()["cus"]
    for min_fill in (1, 0):
        ctx.set_option("min_fill", min_fill)
        assert render(rm, ctx, scene)[1]["workgroups"] == cus
        assert render(rm, ctx, scene, 64, 64)[1]["workgroups"] == 16
    ctx.close()


@pytest.mark.gpu
def test_frames_on_four_streams_with_the_floor_active(rm, monkeypatch):
    """Four streams x three frames at Q = 4 (every launch brings two workgroups per CU, the kernel compiled for the
    configuration takes over at the third): every frame has the serial render's hash."""
    import torch
    ctx, scene = gpu_scene(rm, monkeypatch, 4)
    cus = ctx.last_launch()["cus"]
    ctx.set_option("min_fill", 0)
    serial, shape = render(rm, ctx, scene)
    assert shape["workgroups"] == cus
    want = digest(serial)
    ctx.set_option("min_fill", 1)
    streams = [torch.cuda.Stream(device=torch.device("cuda:0")) for _ in range(4)]
    frames = []
    for f in range(12):
        b, shape = render(rm, ctx, scene, stream=streams[f % 4])
        assert shape["workgroups"] == 2 * cus
        frames.append(b)
    assert [digest(b) for b in frames] == [want] * 12
    ctx.close()
