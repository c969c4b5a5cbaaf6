"""Re-meshing an edited scene (rm_scene_edit_balls, rm_scene_tiles_update_device; include/rm_raymarch.h, "re-meshing an edited
scene") without a GPU: the reuse rule of tests/remesh_model.py is sound against the exact field evaluated in numpy; the balls
of an edit list on a host-only context, its refusals, and that it changes nothing; the refusals of the update entry and their
order; the registers of tiles_update_kernel; the records' sizes.  tests/test_remesh_gpu.py has the device side."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_sparse_model as S  # noqa: E402
import remesh_model as R  # noqa: E402
import scene_edit_model as M  # noqa: E402
import test_build_invariants as B  # noqa: E402  (the resource-usage helper: one device compile per process and variant)

NAN, INF = float("nan"), float("inf")
BOX = ((-2.0, -2.0, -2.0), 4.0)


def axes(shape):
    lo, size = BOX
    return (lo, (size / (shape[0] - 1), 0, 0), (0, size / (shape[1] - 1), 0), (0, 0, size / (shape[2] - 1)))


def exact_field(points, centers, radii):
    """E = min(10, min over the spheres of |p - c| - r) at float32 points [n, 3]: binary64, sqrt form, centres in binary32."""
    p = np.asarray(points, np.float32).astype(np.float64)
    out = np.full(len(p), 10.0)
    for c, r in zip(np.asarray(centers, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(radii, np.float64).reshape(-1)):
        d = p - c
        out = np.minimum(out, np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - r)
    return out


def exact_sparse(vecs, shape, centers, radii, iso=0.0):
    """(slot, list, tiles) of the exact sparse path in numpy."""
    nu, nv, nw = shape
    k, j, i = np.meshgrid(np.arange(nw), np.arange(nv), np.arange(nu), indexing="ij")
    values = exact_field(S._points(*vecs, i, j, k).reshape(-1, 3), centers, radii)
    slot, lst = S.blocks(exact_field(S.centres(*vecs, *shape), centers, radii), iso, S.bound(*vecs, *shape, 1.0))
    return slot, lst, S.tiles(values, *shape, lst)


def random_edits(rng, n):
    """A batch of one to three random SET / INSERT / REMOVE edits on a list of n spheres."""
    edits = []
    for _ in range(int(rng.integers(1, 4))):
        op = ("set", "insert", "remove")[int(rng.integers(0, 3))] if n > 1 else "insert"
        sphere = (tuple(float(x) for x in rng.uniform(-1.8, 1.8, 3).astype(np.float32)), float(rng.uniform(0.05, 0.4)))
        if op == "remove":
            edits.append(("remove", int(rng.integers(0, n))))
            n -= 1
        elif op == "insert":
            edits.append(("insert", int(rng.integers(0, n + 1)), *sphere))
            n += 1
        else:
            edits.append(("set", int(rng.integers(0, n)), *sphere))
    return edits


def test_the_rule_reuses_only_tiles_that_did_not_change():
    """40 random sphere scenes x random edit batches on two small lattices: every block the model reuses holds the same 729
    values in both scenes, bit for bit; over the run some blocks are reused and some kept-before blocks are reached."""
    n_reused = n_reached = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        shape = (17, 17, 17) if seed % 2 == 0 else (25, 21, 19)
        vecs = axes(shape)
        centers, radii = M.random_spheres(int(rng.integers(3, 16)), seed=seed, lo=-1.8, hi=1.8, rmin=0.05, rmax=0.35)
        edits = random_edits(rng, len(radii))
        balls = R.edit_balls(centers, radii, edits)
        after = M.apply_edits(centers, radii, edits)
        old_slot, _, old_tiles = exact_sparse(vecs, shape, centers, radii)
        _, new_list, new_tiles = exact_sparse(vecs, shape, *after)
        flags = R.reused(old_slot, old_tiles, new_list, balls, *vecs, *shape)
        assert len(flags) == len(new_list)
        for r in np.nonzero(flags)[0]:
            assert old_tiles[old_slot[new_list[r]]].tobytes() == new_tiles[r].tobytes(), (seed, int(new_list[r]))
        n_reused += int(flags.sum())
        n_reached += int(((flags == 0) & (old_slot[new_list] >= 0)).sum())
    assert n_reused > 0 and n_reached > 0, (n_reused, n_reached)


def test_the_model_follows_its_own_special_cases():
    """No ball: every block kept before is reused; a block that was not kept, a NaN inside the lattice, a NaN ball and a
    non-finite centre point evaluate; the NaN fill beyond the lattice is skipped by index."""
    shape = (20, 17, 17)  # 3 x 2 x 2 blocks, the last in a one cell wide: its tiles hold the NaN fill
    vecs = axes(shape)
    centers, radii = M.random_spheres(6, seed=3)
    slot, lst, tiles = exact_sparse(vecs, shape, centers, radii)
    assert len(lst) == 12 and np.isnan(tiles).any()
    assert R.reused(slot, tiles, lst, [], *vecs, *shape).tolist() == [1] * 12
    dropped = slot.copy()
    dropped[lst[5]] = -1
    assert R.reused(dropped, tiles, lst, [], *vecs, *shape).tolist() == [1] * 5 + [0] + [1] * 6
    poisoned = tiles.copy()
    poisoned[3, 0] = NAN  # tile point (0, 0, 0) of a block is always inside the lattice
    assert R.reused(slot, poisoned, lst, [], *vecs, *shape).tolist() == [1] * 3 + [0] + [1] * 8
    assert R.reused(slot, tiles, lst, [((0, 0, 0), NAN)], *vecs, *shape).tolist() == [0] * 12
    assert R.reused(slot, tiles, lst, [((NAN, 0, 0), 0.1)], *vecs, *shape).tolist() == [0] * 12
    assert R.reused(slot, tiles, lst, [((50, 50, 50), 0.1)], *vecs, *shape).tolist() == [1] * 12
    assert R.reused(slot, tiles, lst, [((50, 50, 50), 100.0)], *vecs, *shape).tolist() == [0] * 12
    far = ((0, 0, 0), (3e37, 0, 0), (0, 1, 0), (0, 0, 1))  # index 8 b + 4 = 12 overflows binary32 where index 9 does not
    with np.errstate(over="ignore"):
        assert R.reused(np.zeros(2, np.int32), tiles[:1], [0, 1], [], *far, 10, 9, 9).tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------ rm_scene_edit_balls

def edit_array(N, edits):
    arr = (N.rm_sphere_edit * max(1, len(edits)))()
    for k, e in enumerate(edits):
        arr[k].op, arr[k].index = N.EDIT_OPS[e[0]], int(e[1])
        if len(e) > 2:
            arr[k].center[:] = [float(v) for v in np.asarray(e[2], np.float32)]
            arr[k].radius = float(e[3])
    return arr


EDITS = {
    "set": [("set", 17, (0.31, -0.72, 0.05), 0.22)],
    "insert": [("insert", 40, (0.0, 0.0, 0.0), 0.4)],
    "remove": [("remove", 5)],
    "mixed": [("remove", 0), ("set", 38, (0.31, -0.72, 0.05), 0.22), ("insert", 39, (-1.1, 0.4, 0.9), 0.08), ("insert", 40, (0.0, 0.0, 0.0), 0.4),
              ("remove", 40), ("set", 0, (0.0, 0.0, 0.0), 0.4)],
    "none": [],
}


@pytest.mark.parametrize("case", sorted(EDITS))
@pytest.mark.parametrize("accel", [M.BVH, M.OCTREE, M.NONE])
def test_edit_balls_replays_the_edits_and_changes_nothing(rm, accel, case):
    N = rm._native
    start = M.random_spheres(40, seed=11)
    edits = EDITS[case]
    ctx = rm.Context(None)
    ctx.scene_from_spheres(start[0], start[1], accel)
    before = M.snapshot(ctx, False)
    want = R.edit_balls(start[0], start[1], edits)
    assert len(want) == sum(1 if e[0] != "set" else 2 for e in edits)
    got = ctx.edit_balls(edits)
    assert got.dtype == np.dtype(N.BALL_DTYPE) and len(got) == len(want)
    for g, (c, r) in zip(got, want):
        assert g["center"].tobytes() == np.asarray(c, np.float32).tobytes() and g["radius"] == r and g["reserved"] == 0
    # cap 0 and null balls: it only counts; a smaller cap writes that many
    arr, count = edit_array(N, edits), C.c_int32(-1)
    assert N.lib().rm_scene_edit_balls(ctx._h, arr, len(edits), None, 0, C.byref(count)) == N.RM_OK and count.value == len(want)
    if want:
        room = (N.rm_ball * 2)()
        room[1].radius = -7.0
        assert N.lib().rm_scene_edit_balls(ctx._h, arr, len(edits), room, 1, C.byref(count)) == N.RM_OK and count.value == len(want)
        assert room[0].radius == want[0][1] and room[1].radius == -7.0
    M.assert_same(M.snapshot(ctx, False), before, case)
    # ... and the edit itself still applies afterwards, to the list the balls were taken from
    ctx.edit_spheres(edits)
    fresh = rm.Context(None)
    fresh.scene_from_spheres(*M.apply_edits(start[0], start[1], edits), accel)
    M.assert_same(M.snapshot(ctx, False), M.snapshot(fresh, False), case)
    fresh.close()
    ctx.close()


def test_edit_balls_refuses_what_edit_spheres_refuses_in_the_same_order(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    h = ctx._h
    start = M.random_spheres(40, seed=11)
    room, count = (N.rm_ball * 8)(), C.c_int32(0)

    def raw(op=0, index=0, center=(0.0, 0.0, 0.0), radius=0.1, reserved=0):
        e = (N.rm_sphere_edit * 1)()
        e[0].op, e[0].index, e[0].reserved, e[0].radius = op, index, reserved, radius
        e[0].center[:] = center
        return e

    def both(edits, n):
        """(code, text) of the two entries for the same list; the text after a refused rm_set_option, so each is the entry's own"""
        out = []
        for call in (lambda: L.rm_scene_edit_balls(h, edits, n, room, 8, C.byref(count)), lambda: L.rm_scene_edit_spheres(h, edits, n)):
            assert L.rm_set_option(h, b"no_such_option", 1) == N.RM_E_INVALID
            out.append((call(), L.rm_last_error(h).decode()))
        return out

    one = raw()
    assert L.rm_scene_edit_balls(None, one, 1, room, 8, C.byref(count)) == N.RM_E_INVALID
    # its own arguments
    assert L.rm_scene_edit_balls(h, one, 1, room, 8, None) == N.RM_E_INVALID and L.rm_last_error(h) == b"bad ball buffer"
    assert L.rm_scene_edit_balls(h, one, 1, None, 8, C.byref(count)) == N.RM_E_INVALID
    assert L.rm_scene_edit_balls(h, one, 1, room, -1, C.byref(count)) == N.RM_E_INVALID
    # before any scene: argument errors come ahead of RM_E_NO_SCENE
    a, b = both(one, 1)
    assert a == b and a[0] == N.RM_E_NO_SCENE
    a, b = both(raw(op=7), 1)
    assert a == b and a[0] == N.RM_E_INVALID
    ctx.scene_from_spheres(start[0], start[1], M.BVH)
    before = M.snapshot(ctx, False)
    bad = [(None, 1), (one, -1), (raw(op=3), 1), (raw(op=-1), 1), (raw(reserved=1), 1), (raw(op=0, index=40), 1), (raw(op=0, index=-1), 1),
           (raw(op=1, index=41), 1), (raw(op=2, index=40), 1), (raw(op=0, center=(NAN, 0, 0)), 1), (raw(op=1, center=(0, INF, 0)), 1),
           (raw(op=0, radius=NAN), 1), (raw(op=1, radius=INF), 1), (raw(op=7, index=99, reserved=1, radius=NAN), 1),
           (raw(op=0, index=99, reserved=1), 1), (raw(op=0, index=99, radius=NAN), 1)]
    for edits, n in bad:
        count.value = 5
        a, b = both(edits, n)
        assert a == b and a[0] == N.RM_E_INVALID and a[1], (n, a, b)
        assert count.value == 0
    M.assert_same(M.snapshot(ctx, False), before)
    count.value = 5
    assert L.rm_scene_edit_balls(h, raw(op=2, center=(NAN, NAN, NAN), radius=NAN), 1, room, 8, C.byref(count)) == N.RM_OK and count.value == 1
    assert L.rm_scene_edit_balls(h, None, 0, None, 0, C.byref(count)) == N.RM_OK and count.value == 0
    # a preset's sphere list; primitive lists, forests and presets 5 .. 18 are refused as the edit refuses them
    ctx.scene_from_preset(3, M.OCTREE)
    assert L.rm_scene_edit_balls(h, raw(op=0, index=124), 1, room, 8, C.byref(count)) == N.RM_OK and count.value == 2
    assert (room[0].radius, room[1].radius) == (0.15, 0.1) and ctx.scene_info()["preset_index"] == 3
    ident = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    ctx.scene_from_prims([(1, ident, (0.5, 0.5, 0.5))], M.BVH)
    a, b = both(one, 1)
    assert a == b and a[0] == N.RM_E_UNSUPPORTED
    ctx.scene_from_nodes([(0, -1, -1, ident, (0.5,))], [0], M.BVH)
    a, b = both(one, 1)
    assert a == b and a[0] == N.RM_E_UNSUPPORTED
    a, b = both(raw(op=7), 1)  # ... behind the argument errors
    assert a == b and a[0] == N.RM_E_INVALID
    ctx.scene_from_preset(6, M.BVH)
    a, b = both(one, 1)
    assert a == b and a[0] == N.RM_E_UNSUPPORTED
    ctx.close()


# ------------------------------------------------------------------------------------- rm_scene_tiles_update_device: refusals

def test_the_update_entry_keeps_its_order_of_refusals(rm):
    """Through ctypes on a host-only context (no Python-side validation in the way): the code and rm_last_error text of every
    refusal, and which one wins.  Every call is refused before any copy, so no pointer is dereferenced."""
    N = rm._native
    L = N.lib()
    ctx, bare = rm.Context(None), rm.Context(None)
    ctx.scene_from_preset(3, 2)
    buf = np.zeros(1 << 17, np.uint8)
    base = buf.ctypes.data

    def at(offset):
        return C.c_void_p(base + offset)

    lat = N.rm_lattice()
    lat.du[0] = lat.dv[1] = lat.dw[2] = 0.1
    lat.nu = lat.nv = lat.nw = 17  # 8 blocks
    good = dict(lattice=lat, prev_slot=at(0), prev_tiles=at(8192), n_prev=2, balls=at(256), n_balls=3, lst=at(512), k=2, tiles=at(8192 + 2 * 5832),
                reused=at(1024), info=at(2048), c=ctx)
    NO_DEVICE, INVALID = N.RM_E_NO_DEVICE, N.RM_E_INVALID
    HOST = "host-only context: there is no CPU distance path"

    def call(**kw):
        a = dict(good, **kw)
        c = a["c"]
        assert L.rm_set_option(c._h, b"no_such_option", 1) == INVALID
        rc = L.rm_scene_tiles_update_device(c._h, C.byref(a["lattice"]) if a["lattice"] is not None else None, a["prev_slot"], a["prev_tiles"], a["n_prev"],
                                            a["balls"], a["n_balls"], a["lst"], a["k"], a["tiles"], a["reused"], a["info"], None)
        return rc, L.rm_last_error(c._h).decode()

    assert L.rm_scene_tiles_update_device(None, C.byref(lat), at(0), at(8192), 2, at(256), 3, at(512), 2, at(8192 + 2 * 5832), None, None, None) == INVALID
    assert call() == (NO_DEVICE, HOST)
    assert call(reused=None, info=None) == (NO_DEVICE, HOST) and call(balls=None, n_balls=0) == (NO_DEVICE, HOST)
    assert call(k=0, lst=None, tiles=None, prev_slot=None, prev_tiles=None) == (NO_DEVICE, HOST)
    assert call(n_prev=0, prev_tiles=None) == (NO_DEVICE, HOST) and call(k=8, n_prev=8, tiles=at(8192 + 8 * 5832)) == (NO_DEVICE, HOST)
    assert call(n_balls=65536) == (NO_DEVICE, HOST)
    bad_lattice = N.rm_lattice()
    bad_lattice.nu = bad_lattice.nv = bad_lattice.nw = 17
    bad_lattice.du[0] = NAN
    refusals = [
        (dict(lattice=None), None),
        (dict(lattice=bad_lattice), None),
        (dict(k=-1), "n_kept must be in [0, n_blocks]"), (dict(k=9), "n_kept must be in [0, n_blocks]"),
        (dict(n_prev=-1), "n_prev_kept must be in [0, n_blocks]"), (dict(n_prev=9), "n_prev_kept must be in [0, n_blocks]"),
        (dict(n_balls=-1), "n_balls must be in [0, 65536]"), (dict(n_balls=65537), "n_balls must be in [0, 65536]"),
        (dict(lst=None), "null list or tiles"), (dict(tiles=None), "null list or tiles"),
        (dict(prev_slot=None), "null previous slot map"), (dict(prev_tiles=None), "null previous tiles"), (dict(balls=None), "null balls"),
        (dict(lst=at(513)), "list, previous slot map and reused must be 4-byte aligned"),
        (dict(prev_slot=at(2)), "list, previous slot map and reused must be 4-byte aligned"),
        (dict(reused=at(1026)), "list, previous slot map and reused must be 4-byte aligned"),
        (dict(tiles=at(8192 + 2 * 5832 + 4)), "tiles, previous tiles, balls and info must be 8-byte aligned"),
        (dict(prev_tiles=at(8196)), "tiles, previous tiles, balls and info must be 8-byte aligned"),
        (dict(balls=at(260)), "tiles, previous tiles, balls and info must be 8-byte aligned"),
        (dict(info=at(2052)), "tiles, previous tiles, balls and info must be 8-byte aligned"),
        (dict(tiles=at(8192)), "tiles and previous tiles overlap"),
        (dict(tiles=at(8192 + 5832)), "tiles and previous tiles overlap"),
        (dict(tiles=at(8192 + 8), k=1), "tiles and previous tiles overlap"),
        (dict(tiles=at(8192 - 5832 + 8), k=1), "tiles and previous tiles overlap"),
    ]
    for kw, text in refusals:
        for c in (ctx, bare):  # RM_E_INVALID ahead of the device and of the scene
            rc, msg = call(c=c, **kw)
            assert rc == INVALID and (text is None or msg == text) and msg, (kw, rc, msg)
    # which refusal wins: the lattice, then the counts, then the nulls, the alignment, the overlap, the device; the scene last
    assert call(lattice=bad_lattice, k=-1)[1] not in ("", "n_kept must be in [0, n_blocks]")
    assert call(k=-1, n_prev=-1, n_balls=-1, lst=None)[1] == "n_kept must be in [0, n_blocks]"
    assert call(n_prev=-1, n_balls=-1, lst=None)[1] == "n_prev_kept must be in [0, n_blocks]"
    assert call(n_balls=-1, lst=None, tiles=at(8192))[1] == "n_balls must be in [0, 65536]"
    assert call(lst=None, prev_slot=at(2), tiles=at(8192))[1] == "null list or tiles"
    assert call(prev_slot=at(2), tiles=at(8192))[1] == "list, previous slot map and reused must be 4-byte aligned"
    assert call(tiles=at(8192), c=bare)[1] == "tiles and previous tiles overlap"
    assert call(c=bare) == (NO_DEVICE, HOST)
    # buffers that touch without overlapping are fine, and with nothing kept on either side nothing can overlap
    assert call(tiles=at(8192 - 5832), k=1) == (NO_DEVICE, HOST) and call(tiles=at(8192), n_prev=0) == (NO_DEVICE, HOST)
    assert call(tiles=at(8192), k=0) == (NO_DEVICE, HOST)
    for c in (ctx, bare):
        c.close()


# ------------------------------------------------------------------------------------------------------ build and records

@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc not present")
@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_the_update_kernels_spill_no_vgpr_and_use_no_scratch(extra):
    usage = B.resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void tiles_update_kernel<")}
    assert sorted(n.split("(")[0] for n in kernels) == ["void tiles_update_kernel<0>", "void tiles_update_kernel<1>"], sorted(usage)
    B.assert_no_vgpr_spill(kernels)


def test_the_records_have_their_sizes_and_the_entries_their_signatures(rm):
    N = rm._native
    assert C.sizeof(N.rm_ball) == 24 and N.rm_ball.radius.offset == 16 and np.dtype(N.BALL_DTYPE).itemsize == 24
    assert C.sizeof(N.rm_tiles_update_info) == 32
    assert [f for f, _ in N.rm_tiles_update_info._fields_] == ["n_kept", "n_reused", "n_evaluated", "reserved"]
    for name, n_args in (("rm_scene_edit_balls", 6), ("rm_scene_tiles_update_device", 13)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == n_args and hasattr(N.lib(), name), name
    header = open(os.path.join(B.ROOT, "include", "rm_raymarch.h")).read()
    assert "#define RM_TILES_UPDATE_MAX_BALLS 65536" in header and N.RM_TILES_UPDATE_MAX_BALLS == 65536
    assert hasattr(rm, "MeshSession") and hasattr(rm.Context, "mesh_session") and hasattr(rm.Scene, "meshSession")
