"""Option `overlap_fill` ("How many workgroups a launch brings").

`min_fill` is a floor that counts on Q launches overlapping (tests/test_launch_fill.py).  With more streams than hardware queues
they do not, so above the floor a launch of a process with Q < 6 queues brings min(6, ceil(6 / (0.436 Q))) workgroups per CU --
if each of its waves still gets three of the frame's work items.

Host part (no GPU): the rule through rm_debug_overlap_fill against a restatement, the floor entry unchanged, the switch.
GPU part: the bytes with the option on and off, and the grid of a frame that pays for the second stage.

Not here: the issue's GPU tests 1 and 2 (launches whose queue heads are preset so that every workgroup leaves before staging, or
one entry is left per queue).  They test the kernel half of the issue, a workgroup that looks at the queue heads before it
stages; that half measured no gain alone or in combination and was taken out as the issue rules (profiles/NOTES.md, round 6),
so there is no early exit and no preset entry to test."""
import hashlib

import pytest

ENV = "GPU_MAX_HW_QUEUES"
WAVES = 6        # RM_V2_WAVES
CUS = 256        # a host-only context's CU count, and an MI355X's
PER_WAVE = 3     # RM_V2_OVERLAP_ITEMS_PER_WAVE (profiles/NOTES.md, round 6)
QUEUES = [1, 2, 3, 4, 5, 6, 16]


def ceil_div(a, b):
    return -(-a // b)


def floor_rule(asked, q, min_fill=1):
    return max(asked, ceil_div(WAVES, q)) if min_fill else asked


def candidate(asked, q):
    """ceil(6 / E(Q)) with E(Q) = 0.436 Q launches overlapping while the short queues are drained, at most 6; Q >= 6: the floor."""
    if q >= WAVES:
        return floor_rule(asked, q)
    return max(floor_rule(asked, q), min(WAVES, ceil_div(WAVES * 1000, 436 * q)))


def rule(asked, q, items, min_fill=1, overlap=1, cus=CUS):
    floor = floor_rule(asked, q, min_fill)
    if not (min_fill and overlap):
        return floor
    cand = candidate(asked, q)
    if cand <= floor:
        return floor
    waves = 4 * min(ceil_div(items, 4), cus * cand)
    return cand if items >= PER_WAVE * waves else floor


def host_ctx(rm, monkeypatch, q):
    monkeypatch.setenv(ENV, str(q))
    return rm.Context(None)


def test_the_candidates_by_queue_count():
    """What a launch asked for one workgroup per CU brings when its frame is large: Q = 4 is measured, Q = 1, 2, 3, 5 follow the
    same formula, Q >= 6 launches as asked."""
    assert {q: candidate(1, q) for q in QUEUES} == {1: 6, 2: 6, 3: 5, 4: 4, 5: 3, 6: 1, 16: 1}


@pytest.mark.parametrize("queues", QUEUES)
def test_the_rule(rm, monkeypatch, queues):
    """Every (asked, items, overlap_fill, min_fill): items one below and exactly at three per wave of the candidate grid, a frame
    smaller than the grid, and the two frames the issue names (640 x 360 in 64-pixel items: 3 600; 4K in 256-pixel items: 32 640)."""
    ctx = host_ctx(rm, monkeypatch, queues)
    assert ctx.get_option("overlap_fill") == 1 and ctx.get_option("min_fill") == 1
    for min_fill in (1, 0):
        ctx.set_option("min_fill", min_fill)
        for overlap in (1, 0):
            ctx.set_option("overlap_fill", overlap)
            for asked in range(1, 7):
                edge = PER_WAVE * 4 * CUS * candidate(asked, queues)
                for items in (0, 1, 128, 3600, edge - 1, edge, edge + 1, 32640, 10 * edge):
                    assert ctx.overlap_fill(asked, items) == rule(asked, queues, items, min_fill, overlap), (queues, asked, items, min_fill, overlap)
                assert ctx.launch_fill(asked) == floor_rule(asked, queues, min_fill)  # the floor entry: what it returned before
                assert ctx.get_option("blocks_per_cu") == 6  # nothing writes the option
    ctx.set_option("min_fill", 1)
    ctx.set_option("overlap_fill", 1)
    assert ctx.overlap_fill(1, 3600) == floor_rule(1, queues)  # 1.2 items per wave at three per CU: never above the floor
    assert ctx.overlap_fill(1, 32640) == {1: 6, 2: 6, 3: 5, 4: 4, 5: 3, 6: 1, 16: 1}[queues]  # 8 items per wave at Q = 4, 5.3 at six per CU
    for bad in (0, 9, -1):
        with pytest.raises(rm.RmError):
            ctx.overlap_fill(bad, 1000)
    with pytest.raises(rm.RmError):
        ctx.overlap_fill(1, -1)
    ctx.close()


def test_overlap_fill_keeps_the_switch_contract(rm):
    key = "overlap_fill"
    ctx = rm.Context(None)
    others = ("blocks_per_cu", "lds_fill", "min_fill", "item_px", "lpt")
    before = {k: ctx.get_option(k) for k in others}
    assert ctx.get_option(key) == 1
    for probe, stored in [(0, 0), (1, 1), (7, 1), (-1, 1), (0, 0), (1 << 40, 1)]:
        ctx.set_option(key, probe)
        assert ctx.get_option(key) == stored, probe
        assert {k: ctx.get_option(k) for k in others} == before
    ctx.close()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------

NAMES = ("depth", "normal", "sdf", "iters", "rgba")
SENTINEL = 0xAB  # every byte of every buffer before a launch


def gpu_scene(rm, monkeypatch, queues=4, **opts):
    monkeypatch.setenv(ENV, str(queues))  # what the library reads; the HIP runtime of this process started long ago
    ctx = rm.Context(0)
    for k, v in {"item_px": 64, "tile_w": 8, **opts}.items():
        ctx.set_option(k, v)
    scene = rm.Scene("BVH", ctx=ctx)
    scene.loadPreset(3)
    return ctx, scene


def buffers(w, h):
    """The five buffers and the accumulator of one frame, every byte a sentinel."""
    import torch
    dev = torch.device("cuda:0")
    fill = lambda n: torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)  # noqa: E731
    b = dict(depth=fill(w * h), normal=fill(3 * w * h), sdf=fill(2 * w * h).view(torch.int16), iters=fill(2 * w * h).view(torch.int16),
             rgba=fill(4 * w * h), acc=torch.full((4,), -1, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    return b


def render(rm, scene, w, h, b=None, stream=None):
    """One frame with the fused shade and the fused diagnostics, on `stream` (not waited for) or the current one."""
    import torch
    b = b or buffers(w, h)
    with torch.cuda.stream(stream or torch.cuda.current_stream(torch.device("cuda:0"))):
        rm.SphereTracer().runRaymarcher(scene, b["depth"], b["normal"], b["sdf"], b["iters"], w, h, 0.0, shadedBuffer=b["rgba"],
                                        shader="iteration-heatmap", diagnostics=b["acc"])
    return b


def digest(b):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(b"".join(b[k].cpu().numpy().tobytes() for k in NAMES + ("acc",))).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("w, h, item_px", [(640, 360, 64), (1280, 720, 256)])
def test_bytes_do_not_depend_on_the_fill(rm, monkeypatch, w, h, item_px):
    """`overlap_fill` 0 / 1 x `blocks_per_cu` 1 and 6 at Q = 4: one SHA-256 of the five buffers and the diagnostics, that of
    the one-ray-per-lane kernel.  (From the third launch on the wave loop compiled for the configuration renders: the option is
    not part of a configuration.)  Both frames are too small to pay for the second stage -- 3 600 and 3 680 items -- so the grid
    is the floor's, as tests/test_launch_fill.py has it."""
    ctx, scene = gpu_scene(rm, monkeypatch, item_px=item_px)
    cus = ctx.last_launch()["cus"]
    items = (w // 8) * ceil_div(h, item_px // 8)
    got = {}
    for per_cu in (1, 6):
        ctx.set_option("blocks_per_cu", per_cu)
        for overlap in (0, 1):
            ctx.set_option("overlap_fill", overlap)
            b = render(rm, scene, w, h)
            assert "render_kernel_v2<2, true, true, false>" in ctx.last_kernel()
            assert ctx.last_launch()["workgroups"] == min(ceil_div(items, 4), cus * max(per_cu, 2)), (per_cu, overlap)
            got[(per_cu, overlap)] = digest(b)
    ctx.set_option("kernel", 1)
    b = render(rm, scene, w, h)
    assert "render_kernel_v2" not in ctx.last_kernel()
    assert set(got.values()) == {digest(b)}, got
    ctx.close()


@pytest.mark.gpu
def test_a_frame_that_pays_brings_four_workgroups_per_cu(rm, monkeypatch):
    """1 280 x 624 in 64-pixel items is 160 x 78 = 12 480 items: three per wave of 4 x 256 workgroups need 12 288.  At Q = 4,
    one asked: `overlap_fill` 1 launches 4 x CUs workgroups, 0 the floor's 2 x CUs, `min_fill` 0 what was asked; at Q = 16 as
    asked.  Same bytes, those of the one-ray-per-lane kernel; `blocks_per_cu` reads back as set, the LDS request is the same.
    Then twelve frames on four streams, four workgroups per CU each (the kernel compiled for the configuration takes over at the
    third): every frame has that hash."""
    import torch
    w, h = 1280, 624
    ctx, scene = gpu_scene(rm, monkeypatch, blocks_per_cu=1, specialise_v2_after=0)
    cus = ctx.last_launch()["cus"]
    assert cus == CUS and ctx.overlap_fill(1, 160 * 78) == 4 and ctx.overlap_fill(1, 160 * 76) == 2
    got = {}
    for overlap, min_fill, per_cu in ((1, 1, 4), (0, 1, 2), (1, 0, 1)):
        ctx.set_option("overlap_fill", overlap)
        ctx.set_option("min_fill", min_fill)
        b = render(rm, scene, w, h)
        shape = ctx.last_launch()
        assert shape["workgroups"] == per_cu * cus and ctx.get_option("blocks_per_cu") == 1, (overlap, min_fill, shape)
        got[(overlap, min_fill)] = (digest(b), shape["lds_bytes"])
    ctx.set_option("kernel", 1)
    ref = digest(render(rm, scene, w, h))
    assert {v[0] for v in got.values()} == {ref} and len({v[1] for v in got.values()}) == 1
    ctx.close()
    ctx, scene = gpu_scene(rm, monkeypatch, blocks_per_cu=1)
    streams = [torch.cuda.Stream(device=torch.device("cuda:0")) for _ in range(4)]
    frames = [buffers(w, h) for _ in range(12)]
    for f, b in enumerate(frames):
        render(rm, scene, w, h, b, streams[f % 4])
        assert ctx.last_launch()["workgroups"] == 4 * cus
    assert [digest(b) for b in frames] == [ref] * 12 and "compiled in" in ctx.last_kernel()
    ctx.close()
    ctx, scene = gpu_scene(rm, monkeypatch, queues=16, blocks_per_cu=1, specialise_v2_after=0)
    b = render(rm, scene, w, h)
    assert ctx.last_launch()["workgroups"] == cus and digest(b) == ref
    ctx.close()
