"""Sharp meshes on the CPU (rm_scene_sharpen; include/rm_raymarch.h, "sharp meshes"): the numpy model of the rule
(sharp_model.py) over the oracle on a box -- axis-aligned and rotated -- and a sphere, against the exact field E (a single object
under acceleration None: getDistance is E); the Jacobi step against LAPACK; the ABI contract on a host-only context; the build
invariants of every sharp_kernel instantiation.  The bounds are the issue's: measured figures are printed and stand in the
docstrings."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_model as MM  # noqa: E402
import point_model as PM  # noqa: E402
import sharp_model as SM  # noqa: E402

BOX = dict(type="box", pos=(0.03, -0.02, 0.01), half=(0.5, 0.35, 0.25))
ROTATION = (0.4, 0.3, 0.2)


def cube_lattice(n):
    """n^3 points from -1 to 1."""
    step = 2.0 / (n - 1)
    return (-1, -1, -1), (step, 0, 0), (0, step, 0), (0, 0, step), n, n, n


def nets_and_sharp(oracle, prim, n, **knobs):
    """-> (|E| at the surface-nets vertices, |E| at the sharpened ones, the model's SharpResult)."""
    D = PM.oracle_distance(oracle.OracleScene(prims=[prim], accel="None"))
    lat = cube_lattice(n)
    values = SM.lattice_values(D, *lat)
    nets, _, holes = MM.mesh(values, *lat)
    cells = SM.active_cells(values, n, n, n)
    assert holes == 0 and len(cells) == len(nets)
    r = SM.sharpen(D, cells, *lat, **knobs)
    return np.abs(D(nets)[0]), np.abs(D(r.position)[0]), r


@pytest.fixture(scope="module")
def axis_box(oracle):
    return nets_and_sharp(oracle, dict(BOX, rot=None), 17)


def test_edges_and_corners_of_an_axis_aligned_box_lie_on_its_surface(axis_box):
    """17^3: 186 vertices, features 0 / 123 / 55 / 8 for ranks 0 to 3; the 63 vertices of rank 2 or 3 lie within 6e-8 of the box."""
    _, e, r = axis_box
    ranks = np.bincount(r.feature + 1, minlength=5)[1:]
    sharp = r.feature >= 2
    print("axis-aligned box 17^3: ranks", ranks, "largest |E| at rank >= 2: %.3g" % e[sharp].max())
    assert len(e) == 186 and (r.feature >= 0).all()
    assert ranks[2] == 55 and ranks[3] == 8
    assert (e[sharp] <= 1e-6).all(), e[sharp].max()


def test_the_mean_residual_of_an_axis_aligned_box_falls_to_a_quarter_at_least(axis_box):
    """Measured: the mean |E| falls from 1.21e-2 to 3.3e-4 (1 / 36), the largest from 6.3e-2 to 6.7e-3."""
    e0, e, _ = axis_box
    print("axis-aligned box 17^3: mean %.3g -> %.3g, max %.3g -> %.3g" % (e0.mean(), e.mean(), e0.max(), e.max()))
    assert e.mean() <= e0.mean() / 4


@pytest.mark.parametrize("n", [9, 17, 33])
def test_the_mean_residual_of_a_rotated_box_falls_to_a_quarter_at_least(oracle, n):
    """Measured ratios 1 / 27 (9^3), 1 / 20 (17^3), 1 / 7 (33^3); at most 1 vertex (of 69, 281, 1143) falls back to the mean of its
    crossings -- the cap of 1 % keeps the fallback from hiding a failure.  The largest residual stays near the surface nets':
    rank-1 cells that an edge of the box clips without crossing a lattice edge stay wrong (inherent to the method)."""
    e0, e, r = nets_and_sharp(oracle, dict(BOX, rot=ROTATION), n)
    fallback = int((r.feature == 0).sum())
    print("rotated box %d^3: %d vertices, mean %.3g -> %.3g (1 / %.1f), max %.3g -> %.3g, %d at feature 0" %
          (n, len(e), e0.mean(), e.mean(), e0.mean() / e.mean(), e0.max(), e.max(), fallback))
    assert (r.feature >= 0).all()
    assert e.mean() <= e0.mean() / 4
    assert fallback <= 0.01 * len(e)


def test_a_sphere_takes_no_harm(oracle):
    """Measured: the mean |E| goes from 5.9e-3 to 4.9e-3; every vertex is a face (rank 1)."""
    e0, e, r = nets_and_sharp(oracle, dict(type="sphere", pos=BOX["pos"], rot=None, r=0.6), 17)
    print("sphere 17^3: mean %.3g -> %.3g" % (e0.mean(), e.mean()))
    assert e.mean() <= e0.mean()
    assert (r.feature == 1).all()


def test_counts_are_the_evaluations_of_the_rule(axis_box):
    """One primitive: count = 8 corners + (R + 1 + 3) per crossing, here R = 2 and 3 to 7 crossings per cell."""
    _, _, r = axis_box
    per_crossing = 2 + 1 + 3
    assert ((r.count - 8) % per_crossing == 0).all()
    crossings = (r.count - 8) // per_crossing
    assert crossings.min() >= 3 and crossings.max() <= 7


def test_refinement_moves_the_crossings_onto_the_surface(oracle):
    """refine = 0 is the linear crossing of surface nets; each refinement only shrinks the bracket, so the corners of the box get
    no worse and the count per crossing grows by one."""
    _, e0, r0 = nets_and_sharp(oracle, dict(BOX, rot=ROTATION), 9, refine=0)
    _, e8, r8 = nets_and_sharp(oracle, dict(BOX, rot=ROTATION), 9, refine=8)
    assert ((r8.count - 8) * 4 == (r0.count - 8) * 12).all()
    assert e8.mean() <= e0.mean()


# -------------------------------------------------------------------------------------------------------------- Jacobi

def fixed_matrices():
    """Normal matrices sum n n^T of rank 1, 2 and 3 from fixed unit normals, and some with equal and tiny entries."""
    rng = np.random.default_rng(5)
    out = []
    for rank in (1, 2, 3):
        for _ in range(40):
            basis = rng.normal(size=(rank, 3))
            basis /= np.linalg.norm(basis, axis=1, keepdims=True)
            normals = basis[rng.integers(0, rank, 6)] * rng.choice([-1.0, 1.0], 6)[:, None]
            normals = normals.astype(np.float32).astype(np.float64)
            out.append(normals.T @ normals)
    out += [np.diag([3.0, 2.0, 1.0]), np.zeros((3, 3)), np.ones((3, 3)), np.array([[2.0, 1e-9, 0], [1e-9, 2.0, 0], [0, 0, 1.0]]),
            np.array([[4.0, 0, 0], [0, 1.0, 1.0], [0, 1.0, 1.0]])]
    return np.array(out)


def test_six_jacobi_sweeps_find_the_eigenvalues():
    A = fixed_matrices()
    a, V = SM.jacobi(A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2])
    lam = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1)
    want = np.linalg.eigvalsh(A)
    off = max(np.abs(a[:, 0, 1]).max(), np.abs(a[:, 0, 2]).max(), np.abs(a[:, 1, 2]).max())
    print("Jacobi: largest eigenvalue error %.3g, largest off-diagonal term %.3g" % (np.abs(np.sort(lam, axis=1) - want).max(), off))
    assert np.abs(np.sort(lam, axis=1) - want).max() <= 1e-13
    assert off == 0.0
    # V holds the eigenvectors in its columns: orthonormal, and A V = V diag(lam)
    assert np.abs(np.einsum("nki,nkj->nij", V, V) - np.eye(3)).max() <= 1e-13
    assert np.abs(np.einsum("nij,njk->nik", A, V) - V * lam[:, None, :]).max() <= 1e-12
    order = SM.descending(lam)
    sorted_lam = np.take_along_axis(lam, order, axis=1)
    assert (sorted_lam[:, 0] >= sorted_lam[:, 1]).all() and (sorted_lam[:, 1] >= sorted_lam[:, 2]).all()
    ties = SM.descending(np.array([[1.0, 1.0, 1.0], [0.0, 2.0, 2.0], [2.0, 0.0, 2.0]]))
    assert ties.tolist() == [[0, 1, 2], [1, 2, 0], [0, 2, 1]]  # the lower index first


# ------------------------------------------------------------------------------------------------------ ABI contract

def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_lattice(N, shape, origin=(-1, -1, -1), du=(0.25, 0, 0), time=0.0, reserved=0):
    """An rm_lattice filled field by field: make_lattice refuses the counts these tests hand to the library."""
    l = N.rm_lattice()
    for name, v in (("origin", origin), ("du", du), ("dv", (0, 0.25, 0)), ("dw", (0, 0, 0.25))):
        getattr(l, name)[:] = [float(np.float32(x)) for x in v]
    l.nu, l.nv, l.nw = shape
    l.reserved, l.time = reserved, time
    return l


def test_the_library_exports_the_sharp_entries_and_the_query_has_its_size(rm):
    N = rm._native
    assert C.sizeof(N.rm_sharp_query) == 32
    for name in ("rm_mesh_cells_device", "rm_scene_sharpen_device", "rm_scene_sharpen"):
        assert hasattr(N.lib(), name), name


def test_bad_sharpen_arguments_are_invalid_ahead_of_the_device_check(rm):
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)  # host-only, and no scene: every argument check comes first
    NAN, INF = float("nan"), float("inf")
    cells, pos, feat, cnt = np.zeros(4, np.int64), np.zeros((4, 3), np.float32), np.zeros(4, np.int32), np.zeros(4, np.uint32)

    def lat(shape=(9, 9, 9), **more):
        return raw_lattice(N, shape, **more)

    def query(iso=0.0, rank_tol=0.1, reach=1.0, refine=2, reserved=0):
        q = N.rm_sharp_query()
        q.iso, q.rank_tol, q.reach, q.refine, q.reserved = iso, rank_tol, reach, refine, reserved
        return q

    def both(l=None, q=None, n=4, c=vp(cells), p=vp(pos), f=vp(feat), k=vp(cnt), null_lattice=False, null_query=False):
        l = None if null_lattice else C.byref(l or lat())
        q = None if null_query else C.byref(q or query())
        a = L.rm_scene_sharpen(ctx._h, l, q, n, c, p, f, k)
        b = L.rm_scene_sharpen_device(ctx._h, l, q, n, c, p, f, k, None)
        assert a == b, (a, b)
        return a

    # a lattice rm_scene_field refuses
    assert both(null_lattice=True) == N.RM_E_INVALID
    for bad in (dict(shape=(-1, 9, 9)), dict(shape=(9, 65536, 9)), dict(reserved=1), dict(origin=(NAN, 0, 0)), dict(du=(INF, 0, 0)),
                dict(time=NAN), dict(origin=(3e38, 0, 0), du=(3e38, 0, 0))):
        assert both(l=lat(**bad)) == N.RM_E_INVALID, bad
    # the query
    assert both(null_query=True) == N.RM_E_INVALID
    assert both(q=query(reserved=1)) == N.RM_E_INVALID
    for r in (-1, 9, 2 ** 31 - 1):
        assert both(q=query(refine=r)) == N.RM_E_INVALID, r
    for bad in (NAN, INF, -INF):
        assert both(q=query(iso=bad)) == N.RM_E_INVALID
        assert both(q=query(rank_tol=bad)) == N.RM_E_INVALID
        assert both(q=query(reach=bad)) == N.RM_E_INVALID
    assert both(q=query(rank_tol=-1e-9)) == N.RM_E_INVALID and both(q=query(rank_tol=1.0000001)) == N.RM_E_INVALID
    assert both(q=query(reach=-1e-9)) == N.RM_E_INVALID
    # the vertices
    assert both(n=-1) == N.RM_E_INVALID and both(n=2 ** 31) == N.RM_E_INVALID
    assert both(c=None) == N.RM_E_INVALID and both(p=None) == N.RM_E_INVALID
    raw = np.zeros(64, np.uint8)
    assert both(c=C.c_void_p(raw.ctypes.data + 4)) == N.RM_E_INVALID
    for name in ("p", "f", "k"):
        assert both(**{name: C.c_void_p(raw.ctypes.data + 2)}) == N.RM_E_INVALID, name
    assert L.rm_scene_sharpen(None, C.byref(lat()), C.byref(query()), 4, vp(cells), vp(pos), vp(feat), vp(cnt)) == N.RM_E_INVALID
    assert L.rm_scene_sharpen_device(None, C.byref(lat()), C.byref(query()), 4, vp(cells), vp(pos), vp(feat), vp(cnt), None) == N.RM_E_INVALID
    # well formed on a host-only context: no device; feature and count are optional, the limits of the knobs are allowed
    assert both() == N.RM_E_NO_DEVICE
    assert both(f=None, k=None) == N.RM_E_NO_DEVICE
    assert both(n=0, c=None, p=None, f=None, k=None) == N.RM_E_NO_DEVICE
    assert both(q=query(rank_tol=0.0, reach=0.0, refine=0)) == N.RM_E_NO_DEVICE
    assert both(q=query(rank_tol=1.0, refine=8, iso=-0.25)) == N.RM_E_NO_DEVICE
    ctx.scene_from_preset(3, 2)
    assert both() == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.sharpen(cells, (-1, -1, -1), (0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25), (9, 9, 9))
    assert e.value.code == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.sharpen(cells, (-1, -1, -1), (0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25), (9, 9, 9), device=True)
    assert e.value.code == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.mesh((-1, -1, -1), (0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25), (9, 9, 9), sharp=True)
    assert e.value.code == N.RM_E_NO_DEVICE


def test_bad_mesh_cells_arguments_are_invalid_ahead_of_the_device_check(rm):
    """rm_mesh_cells_device: the checks of rm_mesh_field_device, cells in the place of the vertices, 8-byte aligned."""
    N = rm._native
    L = N.lib()
    ctx = rm.Context(None)
    NAN = float("nan")
    vals, cells, info = np.zeros(729, np.float64), np.zeros(8, np.int64), np.zeros(4, np.int64)
    raw = np.zeros(64, np.uint8)

    def lat(shape=(9, 9, 9), **more):
        return raw_lattice(N, shape, **more)

    def call(l=None, v=vp(vals), vt=N.RM_MESH_F64, iso=0.0, c=vp(cells), cap=8, inf=vp(info), null_lattice=False):
        return L.rm_mesh_cells_device(ctx._h, None if null_lattice else C.byref(l or lat()), v, vt, iso, c, cap, inf, None)

    assert call(null_lattice=True) == N.RM_E_INVALID
    for bad in (dict(shape=(-1, 9, 9)), dict(reserved=1), dict(origin=(NAN, 0, 0)), dict(shape=(1025, 1025, 1025))):
        assert call(l=lat(**bad)) == N.RM_E_INVALID, bad
    assert call(v=None) == N.RM_E_INVALID and call(inf=None) == N.RM_E_INVALID
    assert call(iso=NAN) == N.RM_E_INVALID and call(vt=2) == N.RM_E_INVALID and call(vt=-1) == N.RM_E_INVALID
    assert call(cap=-1) == N.RM_E_INVALID and call(c=None, cap=8) == N.RM_E_INVALID
    assert call(c=C.c_void_p(raw.ctypes.data + 4)) == N.RM_E_INVALID
    assert call(v=C.c_void_p(raw.ctypes.data + 4)) == N.RM_E_INVALID and call(inf=C.c_void_p(raw.ctypes.data + 4)) == N.RM_E_INVALID
    assert L.rm_mesh_cells_device(None, C.byref(lat()), vp(vals), N.RM_MESH_F64, 0.0, vp(cells), 8, vp(info), None) == N.RM_E_INVALID
    # well formed: no device; the counting call; a lattice without cells needs no values
    assert call() == N.RM_E_NO_DEVICE and call(c=None, cap=0) == N.RM_E_NO_DEVICE
    assert call(l=lat(shape=(9, 1, 9)), v=None) == N.RM_E_NO_DEVICE
    assert call(v=C.c_void_p(raw.ctypes.data + 4), vt=N.RM_MESH_F32) == N.RM_E_NO_DEVICE
    with pytest.raises(rm.RmError) as e:
        ctx.mesh_cells(vals, (-1, -1, -1), (0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25), (9, 9, 9))
    assert e.value.code == N.RM_E_NO_DEVICE


# ------------------------------------------------------------------------------------------------- build invariants

@pytest.mark.parametrize("extra", [(), ("-DRM_LENGTH_SQRT",)])
def test_sharp_kernels_spill_nothing(extra):
    """Exactly twelve sharp_kernel<ACCEL, GEN> and two sharp_kernel_exact<GEN>: no VGPR spill; no scratch for spheres and
    primitive lists (GEN 0 / 1); the interpreter's per-lane scratch (GEN 2 / 3) within the bound of the other query kernels; the
    static LDS of a workgroup (corner values, crossing records, list and counts) stays below 32 KB."""
    from test_build_invariants import HIPCC, assert_no_vgpr_spill, compiled, resource_usage
    import re
    import shutil
    if not os.path.exists(HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("hipcc / c++filt not present")
    usage = resource_usage(extra, "rm_kernels.hip")
    kernels = {n: r for n, r in usage.items() if n.startswith("void sharp_kernel<")}
    exact = {n: r for n, r in usage.items() if n.startswith("void sharp_kernel_exact<")}
    assert len(kernels) == 12 and len(exact) == 2, sorted(kernels) + sorted(exact)
    assert_no_vgpr_spill(kernels, 800)
    assert_no_vgpr_spill(exact, 800)
    remarks = compiled("rm_kernels.hip", tuple(extra))[0]
    blocks = [b for b in remarks.split("Function Name: ")[1:] if re.match(r"\S*\d+sharp_kernel(_exact)?I", b)]
    lds = [int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) for b in blocks]
    assert len(lds) == 14 and max(lds) <= 32 * 1024, lds
