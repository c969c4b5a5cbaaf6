"""Re-meshing an edited scene on the GPU (rm_scene_tiles_update_device, Context.mesh_session; include/rm_raymarch.h, "re-meshing
an edited scene").  The oracle is the existing code: after every update the session's slot map, list, tiles and mesh must be
the bytes of the full exact sparse path on the same context, and of a second context that uploaded the edited list under
acceleration None with exact = 0.  The flags must be those of tests/remesh_model.py.  No tolerances anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import remesh_model as R  # noqa: E402
import scene_edit_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, OCTREE, BVH = 0, 1, 2
FILL = 0xA5


def axis_lattice(shape):
    return ((-2.0, -2.0, -2.0), (4.0 / (shape[0] - 1), 0, 0), (0, 4.0 / (shape[1] - 1), 0), (0, 0, 4.0 / (shape[2] - 1)), shape)


LATTICES = {
    "A": axis_lattice((65, 65, 65)),  # 512 blocks
    "B": axis_lattice((41, 37, 29)),  # partial last blocks: NaN tile points
    "C": ((-2.0, -2.05, 2.0), (0.125, 0.004, -0.003), (-0.005, 0.125, 0.006), (0.004, -0.003, -0.125), (33, 33, 33)),  # skewed, left-handed
    "D": axis_lattice((97, 97, 97)),  # 1 728 blocks
}


def s300():
    from cpu_raymarcher_amd import synthetic as S
    s = S.synthetic_spheres(300, 300)
    return s[:, :3].astype(np.float32), s[:, 3].copy()


def three():
    """The three-sphere list of tests/test_exact_queries_gpu.py."""
    return np.float32([[0.25, 0, 0], [-0.75, 0.5, 0], [0, -1, 0.5]]), np.array([0.5, 0.25, 0.125])


SCENES = {"grid": M.dense_grid, "s300": s300, "three": three}
# (lattice, scene, acceleration structure)
COMBOS = [("A", "grid", BVH), ("A", "grid", OCTREE), ("A", "grid", NONE), ("A", "s300", OCTREE), ("A", "s300", BVH), ("B", "grid", BVH),
          ("B", "s300", OCTREE), ("C", "grid", OCTREE), ("C", "s300", BVH), ("D", "three", BVH)]


def load(ctx, scene, accel):
    if scene == "grid":
        ctx.scene_from_preset(3, accel)
    else:
        ctx.scene_from_spheres(*SCENES[scene](), accel)
    return SCENES[scene]()


def edit_cases(centers, radii):
    """name -> edit list, for a list of at least three spheres"""
    n = len(radii)
    i = min(7, n - 1)
    c = centers[i].astype(np.float64)
    new = ((0.33, -0.41, 0.27), 0.2)
    return {
        "small_move": [("set", i, c + (0.05, -0.03, 0.02), radii[i])],
        "across": [("set", i, -c + (0.1, 0.0, -0.1), radii[i])],
        "grown": [("set", i, c, 0.8)],
        "insert": [("insert", n // 2, *new)],
        "remove": [("remove", i)],
        "batch": [("set", 0, c * 0.5, 0.3), ("insert", 1, *new), ("remove", 2), ("insert", 0, (-1.2, 1.1, 0.4), 0.12), ("set", 1, (0.9, 0.9, -0.9), 0.25)],
        "nothing": [],
        "outside": [("set", i, (5.0, 5.0, 5.0), radii[i])],
        "remove_all": [("remove", 0)] * n,
    }


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def mesh_of(rm, ctx, lat, slot, lst, k, tiles, iso):
    """rm_mesh_tiles_device over device buffers, the counting call and the filling call -> (vertices, quads, cells, edges) as numpy."""
    import torch
    N = rm._native
    dev = slot.device
    info = torch.zeros(4, dtype=torch.int64, device=dev)

    def call(v, nv, q, nq, c, e):
        N.check(ctx._h, N.lib().rm_mesh_tiles_device(ctx._h, C.byref(lat), C.c_void_p(slot.data_ptr()), ptr(lst) if k else None, k, ptr(tiles) if k else None,
                                                     float(iso), ptr(v), nv, ptr(q), nq, ptr(c), ptr(e), C.c_void_p(info.data_ptr()), None))
    call(None, 0, None, 0, None, None)
    torch.cuda.synchronize()
    nv, nq = (int(x) for x in info.cpu()[:2])
    v = torch.full((nv, 3), 0, dtype=torch.float32, device=dev)
    q = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
    c = torch.zeros(nv, dtype=torch.int64, device=dev)
    e = torch.zeros(nq, dtype=torch.int64, device=dev)
    if nv or nq:
        call(v, nv, q, nq, c, e)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (v, q, c, e))


def full_path(rm, ctx, geom, iso, exact=True):
    """The three device entries of the full sparse path on the active scene -> dict of numpy arrays."""
    import torch
    N = rm._native
    lat = rm.make_lattice(*geom, 0.0)
    with torch.cuda.stream(torch.cuda.default_stream()):
        blocks = ctx.sparse_blocks(*geom, iso=iso, dist=False)
        k = blocks.n_kept
        tiles = torch.full((k, 729), 0.0, dtype=torch.float64, device=blocks.slot.device)
        with ctx._exact(exact):
            N.check(ctx._h, N.lib().rm_scene_tiles_device(ctx._h, C.byref(lat), ptr(blocks.list), k, ptr(tiles), None))
        mesh = mesh_of(rm, ctx, lat, blocks.slot, blocks.list, k, tiles, iso)
    return dict(slot=blocks.slot.cpu().numpy(), list=blocks.list.cpu().numpy(), tiles=tiles.cpu().numpy(), mesh=mesh)


def session_state(rm, ctx, session):
    mesh = mesh_of(rm, ctx, session.lattice, session.slot, session.list, session.n_kept, session.tiles, session.iso)
    return dict(slot=session.slot.cpu().numpy(), list=session.list.cpu().numpy(), tiles=session.tiles.cpu().numpy(), mesh=mesh)


def assert_same_state(got, want, what):
    for key in ("slot", "list", "tiles"):
        assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), (what, key)
    for name, a, b in zip(("vertices", "quads", "cells", "edges"), got["mesh"], want["mesh"]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)


def assert_python_mesh(ctx, session, geom, iso, what):
    """session.mesh(order="tile") against Context.mesh_sparse(exact=True, order="tile")"""
    got, want = session.mesh(order="tile"), ctx.mesh_sparse(*geom, iso=iso, exact=True, order="tile")
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.fixture(scope="module")
def second(rm):
    """The context that uploads the edited list under acceleration None and never sets `exact`."""
    ctx = rm.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("iso", [0.0, 0.05, -0.05])
@pytest.mark.parametrize("lattice,scene,accel", COMBOS)
def test_an_edited_session_holds_the_bytes_of_the_full_exact_path(rm, gpu_ctx, second, lattice, scene, accel, iso):
    ctx, geom = gpu_ctx, LATTICES[lattice]
    seen = set()
    for name in edit_cases(*SCENES[scene]()):
        centers, radii = load(ctx, scene, accel)
        edits = edit_cases(centers, radii)[name]
        session = ctx.mesh_session(*geom, iso=iso)
        stats = session.edit_spheres(edits)
        what = (lattice, scene, accel, iso, name)
        assert stats["n_kept"] == session.n_kept and stats["n_reused"] + stats["n_evaluated"] == stats["n_kept"], what
        assert ctx.get_option("exact") == 0, what
        got = session_state(rm, ctx, session)
        assert_same_state(got, full_path(rm, ctx, geom, iso), what)
        assert_python_mesh(ctx, session, geom, iso, what)
        second.scene_from_spheres(*M.apply_edits(centers, radii, edits), NONE)
        assert_same_state(got, full_path(rm, second, geom, iso, exact=False), what + ("second context",))
        if name == "nothing":
            assert stats["n_reused"] == stats["n_kept"] > 0, what
        if name == "remove_all":
            assert stats["n_kept"] == 0 and len(got["mesh"][0]) == 0, what
        if stats["n_reused"]:
            seen.add("reused")
        if stats["n_evaluated"]:
            seen.add("evaluated")
    assert seen == {"reused", "evaluated"}, (lattice, scene, accel, iso, seen)


def test_the_flags_are_the_models_and_every_category_occurs(rm, gpu_ctx):
    """d_reused against tests/remesh_model.py on the previous tiles read back; over lattices A and D together every category is
    non-empty: reused, evaluated because reached, newly kept, kept then dropped."""
    ctx = gpu_ctx
    totals = dict(reused=0, reached=0, newly_kept=0, dropped=0)
    for lattice, scene, accel, names in (("A", "s300", OCTREE, ("grown", "small_move", "batch")), ("A", "grid", BVH, ("grown", "across")),
                                         ("D", "three", BVH, ("remove", "grown", "outside")), ("B", "grid", BVH, ("insert", "small_move"))):
        geom = LATTICES[lattice]
        for name in names:
            centers, radii = load(ctx, scene, accel)
            edits = edit_cases(centers, radii)[name]
            session = ctx.mesh_session(*geom)
            old_slot, old_tiles = session.slot.cpu().numpy(), session.tiles.cpu().numpy()
            balls = ctx.edit_balls(edits)
            stats = session.edit_spheres(edits)
            new_slot, new_list = session.slot.cpu().numpy(), session.list.cpu().numpy()
            flags = session.reused.cpu().numpy()
            want = R.reused(old_slot, old_tiles, new_list, balls, *geom[:4], *geom[4])
            assert flags.tobytes() == want.tobytes(), (lattice, scene, name, int((flags != want).sum()))
            assert stats == dict(n_kept=len(new_list), n_reused=int(want.sum()), n_evaluated=int(len(want) - want.sum()))
            if lattice in ("A", "D"):
                totals["reused"] += int(want.sum())
                totals["reached"] += int(((want == 0) & (old_slot[new_list] >= 0)).sum())
                totals["newly_kept"] += int((old_slot[new_list] < 0).sum())
                totals["dropped"] += int(((old_slot >= 0) & (new_slot < 0)).sum())
    assert all(v > 0 for v in totals.values()), totals


def test_a_chain_of_six_edits_through_the_ping_pong_buffers(rm, gpu_ctx, second):
    ctx, geom = gpu_ctx, LATTICES["A"]
    centers, radii = load(ctx, "s300", BVH)
    session = ctx.mesh_session(*geom)
    chain = [[("set", 7, (0.2, 0.1, -0.3), 0.3)], [("insert", 0, (-1.0, 1.0, 1.0), 0.25), ("remove", 11)], [("set", 0, (-1.1, 1.0, 1.0), 0.6)],
             [("remove", 0)], [], [("set", 120, (1.2, -1.2, 0.3), 0.05), ("set", 7, (0.2, 0.1, -0.3), 0.02)]]
    for step, edits in enumerate(chain):
        stats = session.edit_spheres(edits)
        centers, radii = M.apply_edits(centers, radii, edits)
        got = session_state(rm, ctx, session)
        assert_same_state(got, full_path(rm, ctx, geom, 0.0), step)
        assert 0 < stats["n_reused"] <= stats["n_kept"], (step, stats)
    second.scene_from_spheres(centers, radii, NONE)
    assert_same_state(got, full_path(rm, second, geom, 0.0, exact=False), "second context")
    assert_python_mesh(ctx, session, geom, 0.0, "chain")


def bounding_ball(d):
    """A ball that contains a primitive of synthetic_mixed_prims: its position and its bounding radius, with room for the
    binary32 roundings of the transform."""
    rho = d["r"] if d["type"] == "sphere" else float(np.linalg.norm(d["half"])) if d["type"] == "box" else d["radius"] * 1.25
    return (np.asarray(d["pos"], np.float32), rho * (1 + 1e-5) + 1e-5)


@pytest.mark.parametrize("accel", [BVH, OCTREE])
@pytest.mark.parametrize("moved", [1, 2])  # a box, a torus
def test_caller_supplied_balls_for_a_rigid_primitive_scene(rm, gpu_ctx, accel, moved):
    from cpu_raymarcher_amd import synthetic as S
    ctx, geom = gpu_ctx, LATTICES["A"]
    prims = S.synthetic_mixed_prims(12)
    ctx.scene_from_prims(S.mixed_prims_as_triples(prims, rm.make_transform), accel)
    session = ctx.mesh_session(*geom)
    after = [dict(d) for d in prims]
    after[moved]["pos"] = [float(np.float32(-v * 0.8 + 0.1)) for v in prims[moved]["pos"]]
    ctx.scene_from_prims(S.mixed_prims_as_triples(after, rm.make_transform), accel)
    stats = session.update([bounding_ball(prims[moved]), bounding_ball(after[moved])])
    assert stats["n_reused"] > 0 and stats["n_evaluated"] > 0, stats
    assert_same_state(session_state(rm, ctx, session), full_path(rm, ctx, geom, 0.0), (accel, moved))
    assert_python_mesh(ctx, session, geom, 0.0, (accel, moved))


def test_the_update_names_its_kernel(rm, gpu_ctx):
    N = rm._native
    ctx, geom = gpu_ctx, LATTICES["B"]
    for general, loader in ((0, lambda: ctx.scene_from_preset(3, OCTREE)),
                            (1, lambda: ctx.scene_from_prims([(1, rm.make_transform(0.1, 0.2, 0.3), (0.5, 0.4, 0.3))], BVH))):
        loader()
        for length in (0, 1):
            ctx.set_option("length", length)  # (the option selects among defined results: a session lives under one value)
            try:
                session = ctx.mesh_session(*geom)
                stats = session.update([((-1.0, -1.0, -1.0), 0.3)])
                assert stats["n_kept"] > 0 and stats["n_reused"] + stats["n_evaluated"] == stats["n_kept"], stats
                name = N.lib().rm_last_kernel(ctx._h).decode()
                assert name == "tiles_update_kernel<%d>" % general + (" [length=sqrt]" if length else ""), name
                assert_same_state(session_state(rm, ctx, session), full_path(rm, ctx, geom, 0.0), (general, length))
            finally:
                ctx.set_option("length", 0)


def test_a_forest_is_unsupported_and_its_buffers_stay_untouched(rm, gpu_ctx):
    import torch
    N = rm._native
    ctx, geom = gpu_ctx, LATTICES["B"]
    lat = rm.make_lattice(*geom, 0.0)
    ident = [1.0 if k % 5 == 0 else 0.0 for k in range(16)]
    ctx.scene_from_nodes([(0, -1, -1, ident, (0.5,))], [0], BVH)
    session = ctx.mesh_session(*geom)  # the full path serves a forest
    assert session.n_kept > 0 and session.stats["n_evaluated"] == session.n_kept
    dev = session.slot.device
    k = session.n_kept
    tiles = torch.full((k, 729), -7.0, dtype=torch.float64, device=dev)
    flags = torch.full((k,), FILL, dtype=torch.int32, device=dev)
    info = torch.full((4,), FILL, dtype=torch.int64, device=dev)
    rc = N.lib().rm_scene_tiles_update_device(ctx._h, C.byref(lat), ptr(session.slot), ptr(session.tiles), k, None, 0, ptr(session.list), k, ptr(tiles),
                                              ptr(flags), ptr(info), None)
    torch.cuda.synchronize()
    assert rc == N.RM_E_UNSUPPORTED and "expression-program" in N.lib().rm_last_error(ctx._h).decode()
    assert bool((tiles == -7.0).all()) and bool((flags == FILL).all()) and bool((info == FILL).all())
    with pytest.raises(rm.RmUnsupported):
        session.update([((0.0, 0.0, 0.0), 0.1)])
    before = session_state(rm, ctx, session)
    session.update(None)
    assert_same_state(session_state(rm, ctx, session), before, "forest, balls=None")
    assert_same_state(before, full_path(rm, ctx, geom, 0.0), "forest")


def test_update_without_balls_resamples_everything(rm, gpu_ctx):
    ctx, geom = gpu_ctx, LATTICES["C"]
    load(ctx, "grid", OCTREE)
    session = ctx.mesh_session(*geom, iso=0.05)
    ctx.scene_from_spheres(*s300(), BVH)  # another scene altogether: no ball describes the change
    stats = session.update(None)
    assert stats == dict(n_kept=session.n_kept, n_reused=0, n_evaluated=session.n_kept) and session.n_kept > 0
    assert_same_state(session_state(rm, ctx, session), full_path(rm, ctx, geom, 0.05), "balls=None")
    assert_python_mesh(ctx, session, geom, 0.05, "balls=None")


def test_the_scene_mirror_routes_edits_through_the_open_session(rm, gpu_ctx):
    geom = LATTICES["B"]
    scene = rm.Scene("BVH", ctx=gpu_ctx)
    scene.loadPreset(3)
    session = scene.meshSession(*geom)
    scene.setSphere(62, (0.07, -0.03, 0.11), 0.3)
    scene.removeSphere(0)
    assert session.stats["n_reused"] > 0 and session.stats["n_evaluated"] > 0
    assert_same_state(session_state(rm, gpu_ctx, session), full_path(rm, gpu_ctx, geom, 0.0), "Scene")
    got, want = session.mesh(triangles=True), scene.toMesh(*geom[:4], shape=geom[4], sparse=True, exact=True, triangles=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    scene.loadPreset(0)
    assert scene._session is None
