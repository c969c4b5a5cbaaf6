"""Sparse meshes (rm_lattice_blocks, rm_scene_blocks_device, rm_scene_tiles_device, rm_mesh_tiles_device, rm_scene_mesh_sparse;
Context.sparse_blocks, mesh_sparse, mesh_box(sparse=True), Scene.toMesh(sparse=True)): the mesh of the dense path from the
8 x 8 x 8-cell blocks near the surface.  CPU tests: the ABI contract on a host-only context, the block counts by hand, the numpy
model of tests/mesh_sparse_model.py against the dense model, the registers of the kernels.  GPU tests: the coarse pass returns
the exact distance of an acceleration-None upload under every acceleration (the pruned walk) and the model's slots; the tiles
hold rm_scene_field's values; the mesher equals the model byte for byte under the capacity protocol, on two streams and on a
second run; the whole path equals Context.mesh byte for byte; the knob acts; the host entry; the Python mirror."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_model as M  # noqa: E402
import mesh_sparse_model as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
FILL = 0xA5
SKEW = ((0.25, -1.5, 0.75), (0.1, 0.013, -0.007), (-0.011, 0.21, 0.017), (0.023, -0.019, 0.37))  # test_scene_mesh.py's: right-handed
AXES = ((-0.35, -0.3, -0.25), (0.1, 0, 0), (0, 0.1, 0), (0, 0, 0.1))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    return np.ascontiguousarray(a).view(np.uint8).tobytes() == np.ascontiguousarray(b).view(np.uint8).tobytes()


def lattice(rm, origin, du, dv, dw, shape, time=0.0):
    lat = rm._native.rm_lattice()
    for name, v in (("origin", origin), ("du", du), ("dv", dv), ("dw", dw)):
        getattr(lat, name)[:] = [float(x) for x in np.asarray(v, np.float32)]
    lat.nu, lat.nv, lat.nw = shape
    lat.time = time
    return lat


def vectors(lat):
    return tuple(np.array(list(getattr(lat, k)), np.float32) for k in ("origin", "du", "dv", "dw")) + (lat.nu, lat.nv, lat.nw)


# ----------------------------------------------------------------------------------------------------- CPU: ABI contract

def test_the_library_exports_the_sparse_entries_and_the_record_has_its_size(rm):
    N = rm._native
    for name in ("rm_lattice_blocks", "rm_scene_blocks_device", "rm_scene_tiles_device", "rm_mesh_tiles_device", "rm_scene_mesh_sparse"):
        assert hasattr(N.lib(), name), name
    assert C.sizeof(N.rm_sparse_info) == 32
    assert [f for f, _ in N.rm_sparse_info._fields_] == ["n_blocks", "n_kept", "reserved"]
    assert N.RM_SPARSE_BLOCK == 8 == S.B
    header = open(os.path.join(ROOT, "include", "rm_raymarch.h")).read()
    assert "#define RM_SPARSE_BLOCK 8" in header


def test_block_counts_by_hand(rm):
    """ceil((n - 1) / 8) blocks on an axis of n points, none below 2 points: 0 -> 0, 1 -> 0, 2 -> 1, 9 -> 1 (8 cells), 10 -> 2
    (9 cells), 17 -> 2 (16 cells), 18 -> 3, 65 535 -> 8 192 (65 534 cells = 8 191 * 8 + 6)."""
    N = rm._native
    want = {0: 0, 1: 0, 2: 1, 9: 1, 10: 2, 17: 2, 18: 3, 65535: 8192}
    step = 1e-4
    for n, nb in want.items():
        assert S.axis_blocks(n) == nb
        for axis in range(3):
            shape = [9, 10, 17]
            shape[axis] = n
            dims = (C.c_int32 * 3)(-1, -1, -1)
            lat = lattice(rm, (0, 0, 0), (step, 0, 0), (0, step, 0), (0, 0, step), tuple(shape))
            assert N.lib().rm_lattice_blocks(C.byref(lat), dims) == N.RM_OK
            expect = [1, 2, 2]
            expect[axis] = nb
            assert list(dims) == expect, (n, axis)
    dims = (C.c_int32 * 3)()
    bad = lattice(rm, (0, 0, 0), (NAN, 0, 0), (0, 1, 0), (0, 0, 1), (9, 9, 9))
    assert N.lib().rm_lattice_blocks(C.byref(bad), dims) == N.RM_E_INVALID
    assert N.lib().rm_lattice_blocks(None, dims) == N.RM_E_INVALID
    assert N.lib().rm_lattice_blocks(C.byref(lattice(rm, *AXES, (9, 9, 9))), None) == N.RM_E_INVALID


def test_bad_sparse_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    ctx.scene_from_preset(3, 2)
    bare = rm.Context(None)  # no scene
    i32 = np.zeros(4096, np.int32)
    f64 = np.zeros(4096, np.float64)
    f32 = np.zeros(4096, np.float32)
    info, sinfo = N.rm_mesh_info(), N.rm_sparse_info()

    def lat(shape=(17, 17, 17), origin=(0, 0, 0), du=(0.1, 0, 0), dv=(0, 0.1, 0), dw=(0, 0, 0.1), time=0.0, reserved=0):
        l = lattice(rm, origin, du, dv, dw, shape, time)
        l.reserved = reserved
        return l

    def ref(l):
        return None if l is None else C.byref(l)

    def blocks(c, l, iso=0.0, lip=1.0, slot=vp(i32), lst=vp(i32), dist=vp(f64), inf=vp(f64)):
        return L.rm_scene_blocks_device(c._h, ref(l), iso, lip, slot, lst, dist, inf, None)

    def tiles(c, l, lst=vp(i32), k=2, out=vp(f64)):
        return L.rm_scene_tiles_device(c._h, ref(l), lst, k, out, None)

    def mesh(c, l, slot=vp(i32), lst=vp(i32), k=2, til=vp(f64), iso=0.0, v=vp(f32), cv=8, q=vp(i32), cq=8, ce=vp(f64), ed=vp(f64), inf=vp(f64)):
        return L.rm_mesh_tiles_device(c._h, ref(l), slot, lst, k, til, iso, v, cv, q, cq, ce, ed, inf, None)

    def host(c, l, iso=0.0, lip=1.0, v=vp(f32), cv=8, q=vp(i32), cq=8, ce=vp(f64), ed=vp(f64), inf=C.byref(info), sinf=C.byref(sinfo)):
        return L.rm_scene_mesh_sparse(c._h, ref(l), iso, lip, v, cv, q, cq, ce, ed, inf, sinf)

    def every(c, l):
        return {blocks(c, l), tiles(c, l, k=0), mesh(c, l, k=0), host(c, l)}

    # everything rm_scene_field refuses about a lattice, with and without a scene
    bad = [dict(shape=(-1, 17, 17)), dict(shape=(17, 65536, 17)), dict(shape=(17, 17, -7)), dict(reserved=1), dict(origin=(NAN, 0, 0)),
           dict(du=(0, INF, 0)), dict(dv=(0, 0, -INF)), dict(dw=(NAN, 0, 0)), dict(time=NAN), dict(time=INF),
           dict(du=(3e38, 0, 0), shape=(3, 17, 17)), dict(origin=(-3e38, 0, 0), dw=(-3e38, 0, 0), shape=(17, 17, 2))]
    for kw in bad:
        for c in (ctx, bare):
            assert every(c, lat(**kw)) == {N.RM_E_INVALID}, kw
    assert every(ctx, None) == {N.RM_E_INVALID}
    small = dict(du=(1e-4, 0, 0), dv=(0, 1e-4, 0), dw=(0, 0, 1e-4))
    # more than 2^24 blocks: 257 * 256 * 256
    for c in (ctx, bare):
        assert every(c, lat(shape=(2050, 2049, 2049), **small)) == {N.RM_E_INVALID}
    # a well-formed 2048 x 2048 x 1025 lattice (2^32 points, 2^23 blocks) and the largest one (2^24 blocks) are accepted
    for shape in ((2048, 2048, 1025), (2049, 2049, 2049), (65535, 9, 9)):
        assert every(ctx, lat(shape=shape, **small)) == {N.RM_E_NO_DEVICE}, shape
    for shape in ((17, 17, 17), (17, 0, 17), (1, 17, 17)):
        l = lat(shape=shape)
        has_blocks = min(shape) >= 2
        for lip in (0.0, -1.0, NAN, INF, -INF):
            assert blocks(ctx, l, lip=lip) == N.RM_E_INVALID and host(ctx, l, lip=lip) == N.RM_E_INVALID, lip
        for iso in (NAN, INF, -INF):
            assert blocks(ctx, l, iso=iso) == N.RM_E_INVALID and mesh(ctx, l, k=0, iso=iso) == N.RM_E_INVALID and host(ctx, l, iso=iso) == N.RM_E_INVALID
        assert mesh(ctx, l, k=0, cv=-1) == N.RM_E_INVALID and mesh(ctx, l, k=0, cq=-1) == N.RM_E_INVALID
        assert host(ctx, l, cv=-1) == N.RM_E_INVALID and host(ctx, l, cq=-1) == N.RM_E_INVALID
        assert mesh(ctx, l, k=0, v=None) == N.RM_E_INVALID and mesh(ctx, l, k=0, q=None) == N.RM_E_INVALID  # a capacity of 8 without a buffer
        assert host(ctx, l, v=None) == N.RM_E_INVALID and host(ctx, l, q=None) == N.RM_E_INVALID
        assert blocks(ctx, l, inf=None) == N.RM_E_INVALID and mesh(ctx, l, k=0, inf=None) == N.RM_E_INVALID and host(ctx, l, inf=None) == N.RM_E_INVALID
        assert blocks(ctx, l, slot=None) == blocks(ctx, l, lst=None) == (N.RM_E_INVALID if has_blocks else N.RM_E_NO_DEVICE)
        assert mesh(ctx, l, k=0, slot=None) == (N.RM_E_INVALID if has_blocks else N.RM_E_NO_DEVICE)
        assert tiles(ctx, l, k=-1) == N.RM_E_INVALID and mesh(ctx, l, k=-1) == N.RM_E_INVALID
        n_blocks = 8 if has_blocks else 0
        assert tiles(ctx, l, k=n_blocks + 1) == N.RM_E_INVALID and mesh(ctx, l, k=n_blocks + 1) == N.RM_E_INVALID
        if has_blocks:
            assert tiles(ctx, l, lst=None) == N.RM_E_INVALID and tiles(ctx, l, out=None) == N.RM_E_INVALID
            assert mesh(ctx, l, lst=None) == N.RM_E_INVALID and mesh(ctx, l, til=None) == N.RM_E_INVALID
            assert tiles(ctx, l, k=8) == N.RM_E_NO_DEVICE and mesh(ctx, l, k=8) == N.RM_E_NO_DEVICE
        for off in (1, 2):
            o32, of32, o64 = C.c_void_p(i32.ctypes.data + off), C.c_void_p(f32.ctypes.data + off), C.c_void_p(f64.ctypes.data + off)
            assert blocks(ctx, l, slot=o32) == N.RM_E_INVALID and blocks(ctx, l, lst=o32) == N.RM_E_INVALID
            assert tiles(ctx, l, k=0, lst=o32) == N.RM_E_INVALID and mesh(ctx, l, k=0, slot=o32) == N.RM_E_INVALID and mesh(ctx, l, k=0, lst=o32) == N.RM_E_INVALID
            assert mesh(ctx, l, k=0, v=of32) == N.RM_E_INVALID and mesh(ctx, l, k=0, q=o32) == N.RM_E_INVALID
            assert host(ctx, l, v=of32) == N.RM_E_INVALID and host(ctx, l, q=o32) == N.RM_E_INVALID
            assert mesh(ctx, l, k=0, v=of32, cv=0) == N.RM_E_INVALID  # alignment is asked of any pointer given
        for off in (1, 2, 4):
            o64 = C.c_void_p(f64.ctypes.data + off)
            assert blocks(ctx, l, dist=o64) == N.RM_E_INVALID and blocks(ctx, l, inf=o64) == N.RM_E_INVALID
            assert tiles(ctx, l, k=0, out=o64) == N.RM_E_INVALID
            for name in ("til", "ce", "ed", "inf"):
                assert mesh(ctx, l, k=0, **{name: o64}) == N.RM_E_INVALID, name
            assert host(ctx, l, ce=o64) == N.RM_E_INVALID and host(ctx, l, ed=o64) == N.RM_E_INVALID
        # well formed: no device; the optional outputs may be null
        assert every(ctx, l) == {N.RM_E_NO_DEVICE}
        assert blocks(ctx, l, dist=None) == N.RM_E_NO_DEVICE and mesh(ctx, l, k=0, ce=None, ed=None) == N.RM_E_NO_DEVICE
        assert mesh(ctx, l, k=0, v=None, cv=0, q=None, cq=0) == N.RM_E_NO_DEVICE  # the counting call
        assert host(ctx, l, v=None, cv=0, q=None, cq=0, ce=None, ed=None, sinf=None) == N.RM_E_NO_DEVICE
    good = lat()
    assert L.rm_scene_blocks_device(None, C.byref(good), 0.0, 1.0, vp(i32), vp(i32), None, vp(f64), None) == N.RM_E_INVALID
    assert L.rm_scene_tiles_device(None, C.byref(good), vp(i32), 0, vp(f64), None) == N.RM_E_INVALID
    assert L.rm_mesh_tiles_device(None, C.byref(good), vp(i32), vp(i32), 0, vp(f64), 0.0, None, 0, None, 0, None, None, vp(f64), None) == N.RM_E_INVALID
    assert L.rm_scene_mesh_sparse(None, C.byref(good), 0.0, 1.0, None, 0, None, 0, None, None, C.byref(info), None) == N.RM_E_INVALID
    # the scene check comes last, and rm_mesh_tiles_device has none
    assert blocks(bare, lat(reserved=1)) == N.RM_E_INVALID and host(bare, good, lip=0.0) == N.RM_E_INVALID
    assert {blocks(bare, good), tiles(bare, good), mesh(bare, good), host(bare, good)} == {N.RM_E_NO_DEVICE}
    for call in (lambda: ctx.mesh_sparse(*AXES, (9, 9, 9)), lambda: ctx.sparse_blocks(*AXES, (9, 9, 9)), lambda: ctx.mesh_box((8, 8, 8), sparse=True)):
        with pytest.raises(rm.RmError) as e:
            call()
        assert e.value.code == N.RM_E_NO_DEVICE


# ------------------------------------------------------------------------------------- CPU: the model against the dense model

def analytic(kind, n, half):
    """test_scene_mesh.py's fields: both are exact distances, so 1-Lipschitz."""
    x = np.linspace(-half, half, n)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    s = 2.0 * half / (n - 1)
    vecs = ((-half,) * 3, (s, 0, 0), (0, s, 0), (0, 0, s))

    def f(p):
        p = np.asarray(p, np.float64)
        if kind == "sphere":
            return np.sqrt((p ** 2).sum(axis=-1)) - 1.5
        return np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 2] ** 2) - 1.0) ** 2 + p[..., 1] ** 2) - 0.4

    return f(np.stack([X, Y, Z], axis=-1)), vecs, f


@pytest.mark.parametrize("kind,n,half,iso", [("sphere", 41, 4.0, 0.0), ("torus", 49, 3.0, 0.0), ("sphere", 36, 4.0, 0.3)])
def test_the_model_equals_the_dense_model_after_sorting_by_the_keys(kind, n, half, iso):
    d, vecs, f = analytic(kind, n, half)
    shape = (n, n, n)
    centres = S.centres(*vecs, *shape)
    assert len(centres) == S.axis_blocks(n) ** 3
    slot, lst = S.blocks(f(centres), iso, S.bound(*vecs, *shape, 1.0))
    assert 0 < len(lst) < len(slot), "some blocks are dropped, some kept"
    assert np.array_equal(slot[lst], np.arange(len(lst))) and (np.diff(lst) > 0).all() and (slot >= 0).sum() == len(lst)
    v, q, cells, edges, holes = S.mesh(d, *vecs, *shape, iso, slot)
    dv, dq, dholes = M.mesh(d, *vecs, *shape, iso)
    assert len(v) == len(dv) > 100 and len(q) == len(dq) > 100 and holes == dholes == 0
    assert not same_bits(v, dv), "the tile order is another order"
    sv, sq = S.sort_dense(v, q, cells, edges)
    assert same_bits(sv, dv) and same_bits(sq, dq)
    assert len(np.unique(cells)) == len(cells) and len(np.unique(edges)) == len(edges)
    # the tiles hold the dense values at their indices and the quiet NaN beyond the lattice
    t = S.tiles(d, *shape, lst)
    idx = S.tile_indices(*shape, lst)
    assert t.shape == (len(lst), 729) and same_bits(t[idx >= 0], d.reshape(-1)[idx[idx >= 0]])
    beyond = t[idx < 0].view(np.uint64)
    assert (beyond == 0x7FF8000000000000).all() and ((n - 1) % 8 == 0 or len(beyond) > 0)
    # dropping a block the surface passes through loses vertices: the keep rule is what keeps the mesh whole
    fewer = slot.copy()
    fewer[block_of_cells(cells[:1], shape)] = -1
    fewer[fewer >= 0] = np.arange((fewer >= 0).sum())
    assert len(S.mesh(d, *vecs, *shape, iso, fewer)[0]) < len(v)


def test_the_bound_by_hand():
    """Steps of 0.5, 0.25 and 0.125 along the axes: R = 4 * (0.5 + 0.25 + 0.125) = 3.5; the corners reach |-8| at most:
    slack = 8 * 2^-20; lipschitz 2 -> 7 + 8 * 2^-20.  A NaN distance keeps its block; a distance at the bound exactly is kept."""
    vecs = ((-8, -1, -1), (0.5, 0, 0), (0, 0.25, 0), (0, 0, 0.125))
    b = S.bound(*vecs, 17, 9, 9, 2.0)
    assert b == 7.0 + 8.0 * 2.0 ** -20
    slot, lst = S.blocks([b + 0.25, np.nextafter(b + 0.25, 100.0), NAN, -b + 0.25, np.nextafter(-b + 0.25, -100.0), 0.0], 0.25, b)
    assert slot.tolist() == [0, -1, 1, 2, -1, 3] and lst.tolist() == [0, 2, 3, 5]


# ------------------------------------------------------------------------------------------------- CPU: build invariants

def test_sparse_kernels_spill_nothing():
    from test_build_invariants import HIPCC, resource_usage
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage((), "rm_mesh_sparse.hip")
    kernels = {n: r for n, r in usage.items() if n.split("(")[0] in ("blocks_scan_kernel", "blocks_scatter_kernel", "mesh_tiles_count_kernel",
                                                                     "mesh_tiles_vertex_kernel", "mesh_tiles_quad_kernel", "mesh_scan_kernel")}
    assert len(kernels) == 6, sorted(usage)
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
    usage = resource_usage((), "rm_kernels.hip")
    coarse = {n: r for n, r in usage.items() if n.startswith("void blocks_kernel<") or n.startswith("void tiles_kernel<")}
    assert len(coarse) == 6 + 12, sorted(coarse)  # GEN 0, 1 with and without the walk, GEN 2, 3 without; ACCEL x GEN
    for name, r in coarse.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        first, second = re.search(r"<(\w+), (\w+)>", name).groups()
        if int(first if "blocks_kernel" in name else second) <= 1:
            assert r["ScratchSize [bytes/lane]"] == 0, (name, r)


# ------------------------------------------------------------------------------------------------------------ GPU tests

@pytest.fixture(scope="module")
def sctx(rm):
    """A context of its own.  Interpreter only, like the field tests': every launch here is ahead-of-time."""
    c = rm.Context(0)
    c.set_option("specialise", 0)
    return c


ACCELS = ("None", "Octree", "BVH")
# lipschitz per scene: the smallest of {1, 2, 4} for which every dense-active cell lies in a kept block on SCENE_LATTICE (the
# three primitive scenes are minima of exact distances: 1; the smooth union's blend is 1-Lipschitz as well and 1 suffices)
SCENES = {"grid": 1.0, "spheres40": 1.0, "prims": 1.0, "smooth": 1.0}


def spheres40():
    rng = np.random.default_rng(40)
    return rng.uniform(-1.5, 1.5, (40, 3)).astype(np.float32), rng.uniform(0.05, 0.25, 40)


def load(rm, oracle, ctx, scene, accel):
    sc = rm.Scene(accel, ctx=ctx)
    if scene == "grid":
        sc.loadPreset(3)
    elif scene == "smooth":
        sc.loadPreset(10)
    elif scene == "spheres40":
        sc.loadSpheres(*spheres40())
    elif scene == "prims":
        sc.loadPrims(oracle.OracleScene(accel="None", prims=oracle.synthetic_mixed_prims(40)).prims())
    else:  # one small sphere near the low corner of the small lattices: far blocks are dropped, rings span blocks
        sc.loadSpheres(np.array([scene], np.float32), np.array([0.3]))
    return sc


def scene_lattice(rm, time=0.0):
    """41 x 37 x 33 points over [-4, 4]^3: 5 x 5 x 4 blocks, the last one on j half a block."""
    return lattice(rm, (-4, -4, -4), (0.2, 0, 0), (0, 8 / 36, 0), (0, 0, 0.25), (41, 37, 33), time)


def t32(n, fill=-7):
    import torch
    return torch.full((max(n, 1),), fill, dtype=torch.int32, device="cuda")


def run_blocks(rm, ctx, lat, iso=0.0, lipschitz=1.0, stream=None):
    """rm_scene_blocks_device -> (slot, list[:n_kept], dist, info) as numpy, plus the device tensors (slot, list)."""
    import torch
    N = rm._native
    nb = int(np.prod(S.lattice_blocks(lat.nu, lat.nv, lat.nw)))
    slot, lst = t32(nb), t32(nb)
    dist = torch.full((max(nb, 1),), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    N.check(ctx._h, N.lib().rm_scene_blocks_device(ctx._h, C.byref(lat), iso, lipschitz, C.c_void_p(slot.data_ptr()), C.c_void_p(lst.data_ptr()),
                                                   C.c_void_p(dist.data_ptr()), C.c_void_p(info.data_ptr()), None))
    torch.cuda.synchronize()
    i = info.cpu().numpy()
    k = int(i[1])
    assert (lst[k:nb].cpu().numpy() == -7).all(), "the list is written up to n_kept only"
    return slot[:nb].cpu().numpy(), lst[:k].cpu().numpy(), dist[:nb].cpu().numpy(), i, (slot, lst)


def run_tiles(rm, ctx, lat, d_list, k):
    import torch
    N = rm._native
    tiles = torch.full((max(k, 1), 729), -7.0, dtype=torch.float64, device="cuda")
    N.check(ctx._h, N.lib().rm_scene_tiles_device(ctx._h, C.byref(lat), C.c_void_p(d_list.data_ptr()), k, C.c_void_p(tiles.data_ptr()), None))
    torch.cuda.synchronize()
    return tiles


def run_mesh(rm, ctx, lat, d_slot, d_list, k, d_tiles, iso, cap_v, cap_q, stream=None, keys=True):
    """One rm_mesh_tiles_device call, the outputs filled with FILL bytes first -> (vertices [cap_v, 3], quads [cap_q, 4], cells
    [cap_v], edges [cap_q], info [4]) as numpy."""
    import torch
    N = rm._native
    sizes = (12 * cap_v, 16 * cap_q, 8 * cap_v if keys else 0, 8 * cap_q if keys else 0, 32)
    bufs = [torch.full((max(s, 8),), FILL, dtype=torch.uint8, device="cuda") for s in sizes]
    ptr = [C.c_void_p(b.data_ptr()) if s else None for b, s in zip(bufs, sizes)]
    s = None if stream is None else C.c_void_p(stream.cuda_stream)
    N.check(ctx._h, N.lib().rm_mesh_tiles_device(ctx._h, C.byref(lat), C.c_void_p(d_slot.data_ptr()), C.c_void_p(d_list.data_ptr()), k,
                                                 C.c_void_p(d_tiles.data_ptr()), iso, ptr[0], cap_v, ptr[1], cap_q, ptr[2], ptr[3], ptr[4], s))
    (torch.cuda.current_stream() if stream is None else stream).synchronize()
    raw = [b.cpu().numpy()[:s] for b, s in zip(bufs, sizes)]
    return (raw[0].view(np.float32).reshape(cap_v, 3), raw[1].view(np.uint32).reshape(cap_q, 4), raw[2].view(np.int64), raw[3].view(np.int64),
            raw[4].view(np.int64))


def full_mesh(rm, ctx, lat, d_slot, d_list, k, d_tiles, iso=0.0):
    """The counting call, then the filling call with exact capacities."""
    _, _, _, _, info = run_mesh(rm, ctx, lat, d_slot, d_list, k, d_tiles, iso, 0, 0)
    out = run_mesh(rm, ctx, lat, d_slot, d_list, k, d_tiles, iso, int(info[0]), int(info[1]))
    assert np.array_equal(info, out[4]) and info[3] == 0
    return out


def scene_field(rm, ctx, lat):
    N = rm._native
    dist = np.zeros(lat.nu * lat.nv * lat.nw, np.float64)
    if dist.size:
        N.check(ctx._h, N.lib().rm_scene_field(ctx._h, C.byref(lat), vp(dist), None, None))
    return dist


def exact_at_centres(rm, oracle, ctx, scene, lat):
    """rm_scene_distance of an acceleration-None upload of the scene at the model's block centres (the scene stays active)."""
    load(rm, oracle, ctx, scene, "None")
    ctx.scene_set_time(lat.time)
    centres = S.centres(*vectors(lat))
    if not len(centres):
        return np.zeros(0)
    return ctx.scene_distance(centres)[0]


def assert_model_mesh(got, want, what):
    for g, w, name in zip(got, want, ("vertices", "quads", "cells", "edges", "info")):
        assert g.shape == w.shape and same_bits(g, w), (what, name, g.shape, w.shape)


def model_mesh(lat, dist, iso, slot):
    v, q, cells, edges, holes = S.mesh(dist, *vectors(lat), iso, slot)
    return v, q, cells, edges, np.array([len(v), len(q), holes, 0], np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_the_coarse_pass_returns_the_exact_distance_and_the_models_slots(rm, oracle, sctx, scene, accel):
    lat = scene_lattice(rm, time=0.3)
    exact = exact_at_centres(rm, oracle, sctx, scene, lat)
    load(rm, oracle, sctx, scene, accel)
    sctx.scene_set_time(1.7)  # the lattice's time rules
    slot, lst, dist, info, _ = run_blocks(rm, sctx, lat, 0.0, SCENES[scene])
    assert same_bits(dist, exact), (scene, accel, int((dist != exact).sum()))
    walk = accel == "BVH" and scene != "smooth"
    gen = {"grid": 0, "spheres40": 0, "prims": 1}.get(scene)
    if gen is not None:
        assert sctx.last_kernel() == "blocks_kernel<%d, %s>" % (gen, "true" if walk else "false")
    else:
        assert sctx.last_kernel() in ("blocks_kernel<2, false>", "blocks_kernel<3, false>")
    want_slot, want_list = S.blocks(exact, 0.0, S.bound(*vectors(lat), SCENES[scene]))
    assert same_bits(slot, want_slot) and same_bits(lst, want_list)
    assert info.tolist() == [100, len(want_list), 0, 0] and 0 < len(want_list) < 100


# (shape, lattice vectors, the centre of the one sphere of radius 0.3): the smallest shapes at which the kernels can go wrong
SMALL = {
    "one-block": ((9, 9, 9), AXES, (0.05, 0.1, 0.15)),
    "one-partial-block": ((8, 8, 8), AXES, (0.05, 0.1, 0.15)),
    "eight-blocks": ((17, 17, 17), AXES, (0.0, 0.1, 0.2)),
    "partial-blocks-clamped-centres": ((20, 13, 10), AXES, (0.4, 0.2, 0.1)),
    "one-cell-axis": ((2, 9, 9), AXES, (-0.3, 0.1, 0.15)),
    "no-cells": ((1, 9, 9), AXES, (-0.3, 0.1, 0.15)),
    # the sphere centred on the corner shared by all eight blocks: quad rings span two and four blocks
    "sphere-on-a-block-corner": ((17, 17, 17), AXES, (0.45, 0.5, 0.55)),
    "skew": ((20, 19, 17), SKEW, (0.6, 0.4, 3.9)),
    "left-handed": ((17, 20, 13), (AXES[0], AXES[2], AXES[1], AXES[3]), (0.45, 0.5, 0.55)),
    "far-blocks-dropped": ((33, 25, 17), AXES, (0.0, 0.0, 0.0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("accel", ("BVH", "Octree"))
@pytest.mark.parametrize("case", sorted(SMALL))
def test_the_three_entries_equal_the_model_on_the_small_shapes(rm, oracle, sctx, case, accel):
    shape, vecs, centre = SMALL[case]
    lat = lattice(rm, *vecs, shape)
    exact = exact_at_centres(rm, oracle, sctx, centre, lat)
    load(rm, oracle, sctx, centre, accel)
    # blocks
    slot, lst, dist, info, (d_slot, d_list) = run_blocks(rm, sctx, lat)
    nb = int(np.prod(S.lattice_blocks(*shape)))
    assert same_bits(dist, exact) and len(slot) == nb
    want_slot, want_list = S.blocks(exact, 0.0, S.bound(*vectors(lat), 1.0))
    assert same_bits(slot, want_slot) and same_bits(lst, want_list) and info.tolist() == [nb, len(want_list), 0, 0]
    k = len(lst)
    if case == "far-blocks-dropped":
        assert 0 < k < nb
    if case == "no-cells":
        assert nb == 0 and k == 0
    # tiles: rm_scene_field's values gathered at the tile indices, the quiet NaN beyond the lattice
    field = scene_field(rm, sctx, lat)
    tiles = run_tiles(rm, sctx, lat, d_list, k)
    if k:
        assert sctx.last_kernel().startswith("tiles_kernel<%d, 0>" % {"BVH": 2, "Octree": 1}[accel])
    got_tiles = tiles.cpu().numpy()[:k]
    want_tiles = S.tiles(field, *shape, lst)
    assert same_bits(got_tiles, want_tiles), case
    if case in ("one-partial-block", "partial-blocks-clamped-centres"):
        assert np.isnan(want_tiles).any()
    # the mesher: the counting call and the filling call, twice
    want = model_mesh(lat, field, 0.0, slot)
    for run in range(2):
        assert_model_mesh(full_mesh(rm, sctx, lat, d_slot, d_list, k, tiles), want, (case, run))
    if k:
        assert sctx.last_kernel() == "mesh_tiles_count_kernel"
    if case not in ("no-cells",):
        assert want[4][0] > 0, "the sphere crosses the lattice"
    if case == "sphere-on-a-block-corner":
        # rings that span two and four blocks: quads whose four vertices lie in 2 and in 4 different blocks
        owner = slot[block_of_cells(want[2], shape)][want[1].astype(np.int64)]  # the slot of every quad's four vertices
        spans = np.array([len(set(r)) for r in owner.tolist()])
        assert (spans == 2).any() and (spans == 4).any()
    # every dense-active cell lies in a kept block here (one exact sphere, lipschitz 1): sorted by the keys it is the dense mesh
    dv, dq, _ = M.mesh(field, *vectors(lat), 0.0)
    sv, sq = S.sort_dense(*want[:4])
    assert same_bits(sv, dv) and same_bits(sq, dq), case


def block_of_cells(cells, shape):
    """the block index of cells given by their fine linear index"""
    nu, nv, _ = shape
    nbu, nbv, _ = S.lattice_blocks(*shape)
    i, j, k = cells % nu, (cells // nu) % nv, cells // (nu * nv)
    return ((k // 8) * nbv + j // 8) * nbu + i // 8


@pytest.mark.gpu
def test_the_capacity_protocol_and_two_streams(rm, oracle, sctx):
    import torch
    shape, vecs, centre = SMALL["partial-blocks-clamped-centres"]
    lat = lattice(rm, *vecs, shape)
    load(rm, oracle, sctx, centre, "BVH")
    slot, lst, _, _, (d_slot, d_list) = run_blocks(rm, sctx, lat)
    k = len(lst)
    tiles = run_tiles(rm, sctx, lat, d_list, k)
    want = model_mesh(lat, scene_field(rm, sctx, lat), 0.0, slot)
    V, Q = int(want[4][0]), int(want[4][1])
    assert V > 40 and Q > 40 and k > 1
    for keys in (True, False):
        for cap_v, cap_q in ((0, 0), (V - 1, Q - 1), (1, 1), (V, 1), (1, Q), (0, Q), (V, 0), (V + 5, Q + 5)):
            v, q, cells, edges, info = run_mesh(rm, sctx, lat, d_slot, d_list, k, tiles, 0.0, cap_v, cap_q, keys=keys)
            assert same_bits(info, want[4]), (cap_v, cap_q)
            nv_, nq_ = min(cap_v, V), min(cap_q, Q)
            assert same_bits(v[:nv_], want[0][:nv_]) and same_bits(q[:nq_], want[1][:nq_]), (cap_v, cap_q)
            assert (v[nv_:].view(np.uint8) == FILL).all() and (q[nq_:].view(np.uint8) == FILL).all(), (cap_v, cap_q)
            if keys:
                assert same_bits(cells[:nv_], want[2][:nv_]) and same_bits(edges[:nq_], want[3][:nq_])
                assert (cells[nv_:].view(np.uint8) == FILL).all() and (edges[nq_:].view(np.uint8) == FILL).all()
    # two calls on two streams, both enqueued before either is waited for: the entry orders the users of its scratch itself
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    N = rm._native
    outs = []
    for st in streams:
        with torch.cuda.stream(st):
            outs.append((torch.full((V, 3), -1.0, dtype=torch.float32, device="cuda"), torch.full((Q, 4), -1, dtype=torch.int32, device="cuda"),
                         torch.full((V,), -1, dtype=torch.int64, device="cuda"), torch.full((Q,), -1, dtype=torch.int64, device="cuda"),
                         torch.full((4,), -1, dtype=torch.int64, device="cuda")))
        st.synchronize()
    for st, o in zip(streams, outs):
        p = [C.c_void_p(t.data_ptr()) for t in o]
        N.check(sctx._h, N.lib().rm_mesh_tiles_device(sctx._h, C.byref(lat), C.c_void_p(d_slot.data_ptr()), C.c_void_p(d_list.data_ptr()), k,
                                                      C.c_void_p(tiles.data_ptr()), 0.0, p[0], V, p[1], Q, p[2], p[3], p[4], C.c_void_p(st.cuda_stream)))
    for st in streams:
        st.synchronize()
    for o in outs:
        assert_model_mesh([t.cpu().numpy() for t in o], want, "stream")


def dense_and_sparse(rm, ctx, lat, iso, lipschitz):
    """-> (dense (v, q), sparse (v, q) in dense order, the field, the slot map) of the active scene."""
    vecs = vectors(lat)
    shape = vecs[4:]
    field = scene_field(rm, ctx, lat)
    slot = run_blocks(rm, ctx, lat, iso, lipschitz)[0]
    # the precondition: on the dense field every dense-active cell lies in a kept block
    dv, dq, _ = M.mesh(field, *vecs, iso)
    sv, sq, cells, _, _ = S.mesh(field, *vecs, iso, np.arange(len(slot), dtype=np.int32))  # every block kept: the dense-active cells
    assert len(sv) == len(dv)
    dropped = slot[block_of_cells(cells, shape)] < 0
    assert not dropped.any(), "FIXTURE: %d dense-active cells lie in dropped blocks at lipschitz %g" % (int(dropped.sum()), lipschitz)
    dense = ctx.mesh(*vecs[:4], shape, iso=iso, time=lat.time)
    sparse = ctx.mesh_sparse(*vecs[:4], shape, iso=iso, time=lat.time, lipschitz=lipschitz)
    assert same_bits(dense[0], dv) and same_bits(dense[1], dq)
    return dense, sparse, field, slot


@pytest.mark.gpu
@pytest.mark.parametrize("accel,iso", [("None", 0.0), ("Octree", 0.0), ("BVH", 0.0), ("None", 0.1)])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_the_whole_path_equals_the_dense_mesh_byte_for_byte(rm, oracle, sctx, scene, accel, iso):
    lat = scene_lattice(rm)
    load(rm, oracle, sctx, scene, accel)
    dense, sparse, field, slot = dense_and_sparse(rm, sctx, lat, iso, SCENES[scene])
    assert (slot < 0).any() and len(dense[0]) > 100 and len(dense[1]) > 100
    assert sparse[0].dtype == np.float32 and sparse[1].dtype == np.uint32
    assert same_bits(sparse[0], dense[0]) and same_bits(sparse[1], dense[1]), (scene, accel, iso)
    # order="tile" is the ABI's order
    vecs = vectors(lat)
    tv, tq = sctx.mesh_sparse(*vecs[:4], vecs[4:], iso=iso, lipschitz=SCENES[scene], order="tile")
    want = model_mesh(lat, field, iso, slot)
    assert same_bits(tv, want[0]) and same_bits(tq, want[1])


@pytest.mark.gpu
def test_lipschitz_acts(rm, oracle, sctx):
    lat = scene_lattice(rm)
    vecs = vectors(lat)
    load(rm, oracle, sctx, "grid", "BVH")
    dense = sctx.mesh(*vecs[:4], vecs[4:])
    # a very large value keeps every block and still equals mesh
    every = sctx.sparse_blocks(*vecs[:4], vecs[4:], lipschitz=1e6)
    assert every.n_kept == 100 == len(every.slot) and every.dims == (5, 5, 4)
    v, q = sctx.mesh_sparse(*vecs[:4], vecs[4:], lipschitz=1e6)
    assert same_bits(v, dense[0]) and same_bits(q, dense[1])
    # 0.05 drops blocks the surface passes through: vertices are lost
    few = sctx.sparse_blocks(*vecs[:4], vecs[4:], lipschitz=0.05)
    assert 0 <= few.n_kept < sctx.sparse_blocks(*vecs[:4], vecs[4:]).n_kept < 100
    v2, q2 = sctx.mesh_sparse(*vecs[:4], vecs[4:], lipschitz=0.05)
    assert len(v2) < len(dense[0]) and len(q2) < len(dense[1])


@pytest.mark.gpu
def test_the_host_entry_equals_the_device_path_and_has_no_side_effects(rm, oracle, sctx):
    import torch
    N = rm._native
    lat = scene_lattice(rm, time=0.4)
    sc = load(rm, oracle, sctx, "smooth", "None")
    sctx.scene_set_time(0.9)
    acc = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    sctx._attach_diag(acc)
    slot, lst, _, _, (d_slot, d_list) = run_blocks(rm, sctx, lat, 0.1, 1.0)
    tiles = run_tiles(rm, sctx, lat, d_list, len(lst))
    want = full_mesh(rm, sctx, lat, d_slot, d_list, len(lst), tiles, 0.1)
    V, Q = int(want[4][0]), int(want[4][1])
    assert V > 100 and Q > 100
    info, sinfo = N.rm_mesh_info(-1, -1, -1, -1), N.rm_sparse_info(-1, -1)
    N.check(sctx._h, N.lib().rm_scene_mesh_sparse(sctx._h, C.byref(lat), 0.1, 1.0, None, 0, None, 0, None, None, C.byref(info), C.byref(sinfo)))
    assert (info.n_vertices, info.n_quads, info.n_holes, info.reserved) == (V, Q, 0, 0)
    assert (sinfo.n_blocks, sinfo.n_kept, list(sinfo.reserved)) == (100, len(lst), [0, 0])
    for cap_v, cap_q, keys in ((V + 3, Q + 3, True), (V, Q, False), (V // 2, Q // 3, True)):
        v, q = np.full((cap_v, 3), -1, np.float32), np.full((cap_q, 4), 7, np.uint32)
        cells, edges = np.full(cap_v, -1, np.int64), np.full(cap_q, -1, np.int64)
        info2 = N.rm_mesh_info()
        N.check(sctx._h, N.lib().rm_scene_mesh_sparse(sctx._h, C.byref(lat), 0.1, 1.0, vp(v), cap_v, vp(q), cap_q, vp(cells) if keys else None,
                                                      vp(edges) if keys else None, C.byref(info2), None))
        assert bytes(info2) == bytes(info)
        nv_, nq_ = min(cap_v, V), min(cap_q, Q)
        assert same_bits(v[:nv_], want[0][:nv_]) and same_bits(q[:nq_], want[1][:nq_]) and (v[nv_:] == -1).all() and (q[nq_:] == 7).all()
        if keys:
            assert same_bits(cells[:nv_], want[2][:nv_]) and same_bits(edges[:nq_], want[3][:nq_]) and (cells[nv_:] == -1).all()
    # a lattice without blocks: zero totals
    flat = lattice(rm, *AXES, (1, 9, 9))
    info3, sinfo3 = N.rm_mesh_info(7, 7, 7, 7), N.rm_sparse_info(7, 7)
    N.check(sctx._h, N.lib().rm_scene_mesh_sparse(sctx._h, C.byref(flat), 0.0, 1.0, None, 0, None, 0, None, None, C.byref(info3), C.byref(sinfo3)))
    assert (info3.n_vertices, info3.n_quads, info3.n_holes, sinfo3.n_blocks, sinfo3.n_kept) == (0, 0, 0, 0, 0)
    # no side effects: the armed accumulator was not fired, rm_scene_set_time's value is kept
    torch.cuda.synchronize()
    assert torch.equal(acc, torch.full((4,), -1, dtype=torch.int64, device="cuda")), "a sparse entry fired the diagnostics"
    pts = S.centres(*vectors(lat))[:32]
    at_09 = sctx.scene_distance(pts)[0]
    sctx.scene_set_time(0.9)
    assert same_bits(at_09, sctx.scene_distance(pts)[0])
    W, H = 32, 16  # the armed accumulator is consumed by a render, as after the dense entries
    bufs = [torch.zeros(W * H, dtype=torch.uint8, device="cuda"), torch.zeros(3 * W * H, dtype=torch.uint8, device="cuda"),
            torch.zeros(W * H, dtype=torch.int16, device="cuda"), torch.zeros(W * H, dtype=torch.int16, device="cuda")]
    rm.SphereTracer().runRaymarcher(sc, *bufs, W, H, 0.0)
    torch.cuda.synchronize()
    assert sctx.decode_acc(acc)["total_sdf"] == int(bufs[2].cpu().numpy().view(np.uint16).astype(np.int64).sum())


@pytest.mark.gpu
def test_the_host_entry_on_a_fresh_context_grows_the_scratch_between_its_steps(rm, oracle, sctx):
    """The first mesh call of a context whose scratch is empty: the coarse pass reserves a few kilobytes, the tiles and the
    outputs need far more, so the slot map and the list cross the host while the scratch grows.  Everything equals the three
    device entries on the module's context, byte for byte."""
    N = rm._native
    lat = scene_lattice(rm, time=0.4)
    load(rm, oracle, sctx, "smooth", "None")
    _, lst, _, binfo, (d_slot, d_list) = run_blocks(rm, sctx, lat, 0.1, 1.0)
    want = full_mesh(rm, sctx, lat, d_slot, d_list, len(lst), run_tiles(rm, sctx, lat, d_list, len(lst)), 0.1)
    V, Q = int(want[4][0]), int(want[4][1])
    assert V > 100 and Q > 100 and int(binfo[0]) == 100
    with rm.Context(0) as fresh:
        fresh.set_option("specialise", 0)
        load(rm, oracle, fresh, "smooth", "None")
        v, q = np.full((V, 3), -1, np.float32), np.full((Q, 4), 7, np.uint32)
        cells, edges = np.full(V, -1, np.int64), np.full(Q, -1, np.int64)
        info, sinfo = N.rm_mesh_info(-1, -1, -1, -1), N.rm_sparse_info(-1, -1)
        N.check(fresh._h, N.lib().rm_scene_mesh_sparse(fresh._h, C.byref(lat), 0.1, 1.0, vp(v), V, vp(q), Q, vp(cells), vp(edges), C.byref(info),
                                                       C.byref(sinfo)))
    assert_model_mesh((v, q, cells, edges, np.frombuffer(bytes(info), np.int64)), want, "fresh context")
    assert bytes(sinfo) == binfo.tobytes()


@pytest.mark.gpu
def test_every_stage_of_the_epilogue_at_once_dense_against_sparse(rm, oracle, sctx):
    """Sharp vertices, the winding flip of a left-handed lattice, triangles and the attribute pass with a snap, all in one call:
    `mesh` against `mesh_sparse(order="dense")`, as numpy arrays and as device tensors."""
    load(rm, oracle, sctx, "grid", "BVH").updateTime(0.0)
    vecs = vectors(scene_lattice(rm))
    left, lshape = (vecs[0], vecs[2], vecs[1], vecs[3]), (vecs[5], vecs[4], vecs[6])
    for device in (False, True):
        more = dict(triangles=True, attributes=True, snap=2, sharp=True, device=device)
        a, b = sctx.mesh(*left, lshape, **more), sctx.mesh_sparse(*left, lshape, order="dense", **more)
        assert len(a) == len(b) == 4
        if device:
            assert all(t.is_cuda for t in a + b)
            a, b = [t.cpu().numpy() for t in a], [t.cpu().numpy() for t in b]
        assert len(a[0]) > 100 and a[1].shape == (len(a[1]), 3)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and same_bits(x, y)


@pytest.mark.gpu
def test_the_python_mirror(rm, oracle, sctx):
    sc = load(rm, oracle, sctx, "grid", "BVH")
    sc.updateTime(0.0)
    # mesh_box(sparse=True) is mesh_box, byte for byte, and so is Scene.toMesh(sparse=True)
    bv, bq = sctx.mesh_box((40, 40, 40), margin=2.0)
    sv, sq = sctx.mesh_box((40, 40, 40), margin=2.0, sparse=True)
    assert len(bv) > 1000 and same_bits(sv, bv) and same_bits(sq, bq)
    tv, tq = sc.toMesh(cells=(40, 40, 40), margin=2.0, sparse=True, lipschitz=1.0)
    assert same_bits(tv, bv) and same_bits(tq, bq)
    lat = scene_lattice(rm)
    vecs = vectors(lat)
    ev, eq = sc.toMesh(*vecs[:4], shape=vecs[4:], sparse=True)
    dv, dq = sc.toMesh(*vecs[:4], shape=vecs[4:])
    assert same_bits(ev, dv) and same_bits(eq, dq)
    # triangles, device tensors, attributes: as mesh
    a = sctx.mesh_sparse(*vecs[:4], vecs[4:], triangles=True, attributes=True, snap=2)
    b = sctx.mesh(*vecs[:4], vecs[4:], triangles=True, attributes=True, snap=2)
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and same_bits(x, y)
    d = sctx.mesh_sparse(*vecs[:4], vecs[4:], device=True)
    assert d[0].is_cuda and d[1].is_cuda and same_bits(d[0].cpu().numpy(), dv) and same_bits(d[1].cpu().numpy(), dq)
    # a left-handed lattice gets the winding flip mesh gives it
    left = (vecs[0], vecs[2], vecs[1], vecs[3])
    lshape = (vecs[5], vecs[4], vecs[6])
    lv, lq = sctx.mesh_sparse(*left, lshape)
    mv, mq = sctx.mesh(*left, lshape)
    assert same_bits(lv, mv) and same_bits(lq, mq)
    with pytest.raises(ValueError):
        sctx.mesh_sparse(*vecs[:4], vecs[4:], order="other")
