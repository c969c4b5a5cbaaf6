"""One rm_ctx per GPU (include/rm_raymarch.h "Threading"): owns the device-resident scene."""
import collections
import contextlib
import ctypes as C

import numpy as np

from . import _native as N

# what Context.points returns
Points = collections.namedtuple("Points", "position dist normal object steps count")
SparseBlocks = collections.namedtuple("SparseBlocks", "slot list dist n_kept dims")
Sharp = collections.namedtuple("Sharp", "position feature count")
MeasureWorld = collections.namedtuple("MeasureWorld", "cell_volume volume centroid second projected_area area_estimate")


class Measure(collections.namedtuple("Measure", "n_points n_inside n_nonfinite sum1 sum2 crossings lo hi n_blocks n_kept n_blocks_inside")):
    """rm_measure (include/rm_raymarch.h, "measures") as Python ints -- sum1, sum2, crossings, lo and hi as tuples --, what
    Context.measure_field, Context.measure and MeshSession.measure return.  Two measures compare equal when these integer
    fields are.  `world`: the MeasureWorld rm_measure_world makes of it on the measured lattice."""
    world = None

    def inertia(self):
        """The inertia tensor of the solid about its centroid at unit density, trace(second) * I - second, float64 [3, 3]."""
        xx, yy, zz, xy, yz, zx = self.world.second
        second = np.array([[xx, xy, zx], [xy, yy, yz], [zx, yz, zz]], np.float64)
        return np.trace(second) * np.eye(3) - second


class Parts:
    """What Context.label_field, Context.parts and Scene.parts return (include/rm_raymarch.h, "parts"): `labels` int32
    [nw, nv, nu] -- a numpy array, or a CUDA tensor with device=True --, the part's number at every point of the set and -1
    elsewhere; `n_points`, `n_set`, `n_parts`; `measures`: the Measure of each of the first min(n_parts, records) parts, each
    with `.world` and `.inertia()`; `iso` and `side` as they were asked."""

    def __init__(self, labels, n_points, n_set, n_parts, measures, iso=0.0, side="inside"):
        self.labels, self.n_points, self.n_set, self.n_parts, self.measures = labels, int(n_points), int(n_set), int(n_parts), list(measures)
        self.iso, self.side = float(iso), side

    def by_size(self):
        """The numbers of the parts that have a Measure, the largest (most points) first, ties by number."""
        return sorted(range(len(self.measures)), key=lambda p: (-self.measures[p].n_inside, p))

    def touches_border(self, p):
        """Whether part p has a point on the lattice's border: its index box reaches it.  (An enclosed void is an outside
        part that does not.)"""
        nw, nv, nu = (int(x) for x in self.labels.shape)
        m = self.measures[p]
        return any(lo == 0 or hi == n - 1 for lo, hi, n in zip(m.lo, m.hi, (nu, nv, nw)))

    def select(self, values, keep):
        """A copy of `values` (numpy or torch, shaped or flat, the volume that was labelled) in which every point of the set
        whose part is not in `keep` is mirrored to the other side of iso: 2 * iso - value in the values' own type, so a value
        equal to iso stays iso (and NaN stays NaN: both only occur in an outside set).  `mesh_field` of the result meshes the kept parts only: two
        parts are never adjacent, so every lattice edge that crosses at a kept part keeps both its values, and no kept part's
        vertices or quads change.  torch plumbing, not a kernel."""
        import torch
        if _is_torch(values):
            v = values
            lab = self.labels if _is_torch(self.labels) else torch.from_numpy(np.ascontiguousarray(self.labels))
            lab = lab.to(v.device).reshape(v.shape)
            kept = torch.isin(lab, torch.as_tensor(sorted(int(p) for p in keep), dtype=lab.dtype, device=v.device))
            drop = (lab >= 0) & ~kept
            return torch.where(drop, 2 * self.iso - v, v)
        v = np.asarray(values)
        lab = (self.labels.cpu().numpy() if _is_torch(self.labels) else np.asarray(self.labels)).reshape(v.shape)
        drop = (lab >= 0) & ~np.isin(lab, sorted(int(p) for p in keep))
        return np.where(drop, (2 * self.iso - v).astype(v.dtype, copy=False), v)


class Edt:
    """What Context.edt_field, Context.edt and Scene.edt return (include/rm_raymarch.h, "distances"): `d2` int32 [nw, nv, nu]
    -- a numpy array, or a CUDA tensor with device=True --, the squared index distance of every point of the set to the
    nearest lattice point that is not in it, 0 outside the set, RM_EDT_FAR everywhere when nothing is outside it; `n_points`,
    `n_set`, `max_d2`, `argmax` (linear index, -1 for an empty set) and `at`, the same as (i, j, k) or None; `side` as it was
    asked; `step`: what an index step is worth in the world where the lattice is cubic (rm_lattice_cubic), else None."""

    def __init__(self, d2, n_points, n_set, max_d2, argmax, side="inside", step=None):
        self.d2, self.n_points, self.n_set, self.max_d2, self.argmax = d2, int(n_points), int(n_set), int(max_d2), int(argmax)
        self.side, self.step = side, (None if step is None else float(step))
        nw, nv, nu = (int(x) for x in d2.shape)
        self.at = None if self.argmax < 0 else (self.argmax % nu, self.argmax // nu % nv, self.argmax // (nu * nv))

    def _cubic_step(self):
        if self.step is None:
            raise ValueError("the lattice is not cubic (rm_lattice_cubic): index distances are not world distances")
        return self.step

    def distance(self):
        """sqrt(d2) * step in float64, in `d2`'s container; inf where d2 is RM_EDT_FAR.  Raises on a lattice that is not cubic."""
        step = self._cubic_step()
        if _is_torch(self.d2):
            import torch
            d = torch.sqrt(self.d2.to(torch.float64)) * step
            return torch.where(self.d2 == N.RM_EDT_FAR, torch.full_like(d, float("inf")), d)
        return np.where(self.d2 == N.RM_EDT_FAR, np.inf, np.sqrt(self.d2.astype(np.float64)) * step)

    @property
    def inradius(self):
        """The radius of the largest ball about a lattice point of the set that holds no lattice point outside it: sqrt(max_d2) * step
        (inf when nothing is outside the set)."""
        step = self._cubic_step()
        return float("inf") if self.max_d2 == N.RM_EDT_FAR else float(np.sqrt(np.float64(self.max_d2)) * step)

    def eroded(self, r2):
        """The set eroded by the squared index radius r2 as a volume of `d2`'s container and shape: -1.0 where the point is in
        the set and d2 >= r2, +1.0 elsewhere (float64) -- ready for label_field, mesh_field, measure_field or edt_field at iso = 0."""
        if _is_torch(self.d2):
            import torch
            keep = (self.d2 > 0) & (self.d2 >= int(r2))
            return torch.where(keep, -1.0, 1.0).to(torch.float64)
        return np.where((self.d2 > 0) & (self.d2 >= int(r2)), -1.0, 1.0)

    def max_by_part(self, parts):
        """The largest d2 of each part of `parts` (a Parts of the same lattice and set): int64 [n_parts], in the container of
        `d2` -- torch scatter_reduce on the device, numpy on the host."""
        labels = parts.labels
        if _is_torch(self.d2):
            import torch
            lab = labels if _is_torch(labels) else torch.from_numpy(np.ascontiguousarray(labels))
            lab = lab.to(self.d2.device).reshape(-1).to(torch.int64)
            d = self.d2.reshape(-1).to(torch.int64)
            sel = lab >= 0
            out = torch.zeros(parts.n_parts, dtype=torch.int64, device=self.d2.device)
            return out.scatter_reduce(0, lab[sel], d[sel], reduce="amax", include_self=True)
        lab = (labels.cpu().numpy() if _is_torch(labels) else np.asarray(labels)).reshape(-1)
        d = self.d2.reshape(-1).astype(np.int64)
        out = np.zeros(parts.n_parts, np.int64)
        sel = lab >= 0
        np.maximum.at(out, lab[sel], d[sel])
        return out


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(x):
    """void* of a numpy array (host) or a torch tensor (device); None -> NULL."""
    if x is None:
        return None
    if _is_torch(x):
        return C.c_void_p(x.data_ptr())
    return x.ctypes.data_as(C.c_void_p)


_BPP = {"depth": 1, "normal": 3, "sdf": 2, "iters": 2, "rgba": 4}


_MIXED = "buffers must be all on the host or all on the device"


def _describe(name, x):
    """The C ABI takes raw pointers: what it assumes about a buffer is read here, in one place.  A torch tensor or
    a numpy array -> (on the device, C-contiguous, bytes per element, bytes, writable).  (A plain tuple: these checks are
    host time on every call, and a named one costs half a microsecond per buffer.)"""
    if _is_torch(x):
        e = x.element_size()
        return x.is_cuda, x.is_contiguous(), e, x.numel() * e, True
    if isinstance(x, np.ndarray):
        f = x.flags
        return False, f["C_CONTIGUOUS"], x.itemsize, x.nbytes, f["WRITEABLE"]
    raise ValueError("%s must be a numpy array or a torch tensor, not %s" % (name, type(x).__name__))


def _bytes_on(device, x):
    """The bytes of `x` when it is a contiguous CUDA tensor (device) or a writable contiguous numpy array (not device), else -1."""
    try:
        on_dev, contiguous, _, nbytes, writable = _describe("", x)
    except ValueError:
        return -1
    return nbytes if on_dev == device and contiguous and writable and (device or isinstance(x, np.ndarray)) else -1


def _check_buffers(npx, bufs, need_device=None):
    """bufs: name -> buffer or None.  Every buffer must be C-contiguous, of the reference's element size (depth / normal / rgba
    1 byte, sdf / iters 2 bytes: Uint8ClampedArray / Uint16Array) and hold at least npx pixels; all of them on the host or
    all on one device.  Returns True when they are device (torch CUDA) buffers."""
    on_dev = None
    for name, b in bufs.items():
        if b is None:
            continue
        esz = 2 if name in ("sdf", "iters") else 1
        dev, contiguous, itemsize, nbytes, writable = _describe(name, b)
        if not writable and name != "_in":
            raise ValueError("%s buffer is read-only" % name)
        if not contiguous:
            raise ValueError("%s buffer must be C-contiguous" % name)
        if itemsize != esz and not (dev and itemsize == 1):  # device side: byte views into a packed gather buffer are fine
            raise ValueError("%s buffer must have %d-byte elements (got %d)" % (name, esz, itemsize))
        if nbytes < npx * _BPP[name]:
            raise ValueError("%s buffer holds %d bytes, the tile needs %d" % (name, nbytes, npx * _BPP[name]))
        if on_dev is None:
            on_dev = dev
        elif on_dev != dev:
            raise ValueError(_MIXED)
    if need_device is not None and on_dev is not None and on_dev != need_device:
        raise ValueError("this entry point takes %s buffers" % ("device" if need_device else "host"))
    return bool(on_dev)


def _check_records(name, buf, each, n_frames, on_dev):
    """A buffer of one record of `each` bytes per frame (rm_compare_stats 128, rm_frame_hist 2 128), on the side the pixel
    buffers are on (on_dev None: either).  Returns its side."""
    try:
        dev, contiguous, _, nbytes, _ = _describe(name, buf)
    except ValueError:
        raise ValueError("%s must be a numpy array or a torch tensor" % name) from None
    if not contiguous or nbytes < each * max(0, n_frames):
        raise ValueError("%s must be a contiguous buffer of %d bytes per frame" % (name, each))
    if on_dev is not None and on_dev != dev:
        raise ValueError(_MIXED)
    return dev


def _check_pixel_sets(npx, bufs, rgba, stats, n_frames):
    """_check_buffers for compare_frames: bufs maps depth_a .. iters_b to buffers or None.  Returns True for device buffers."""
    on_dev = None
    for name, b in list(bufs.items()) + [("rgba", rgba)]:
        if b is None:
            continue
        d = _check_buffers(npx, {name.split("_")[0]: b})
        if on_dev is not None and on_dev != d:
            raise ValueError(_MIXED)
        on_dev = d
    if stats is not None:
        on_dev = _check_records("stats", stats, 128, n_frames, on_dev)
    return bool(on_dev)


def _compare_map(map):
    """A name of COMPARE_MAPS or an rm_compare_map value -> the value."""
    return N.COMPARE_MAPS[map] if isinstance(map, str) else int(map)


def percentile(record, permille):
    """The header's percentile rule on a decoded record (an entry of Context.decode_hists(...)[k]["sdf" | "iters"]): any further
    percentile from one read-back.  permille 0 .. 1000 -> (lo, hi), the value range of the bin that holds the pixel of rank
    floor(permille * (pixels - 1) / 1000), clipped to [min, max] as range_lo and range_hi are; (0, 0) without pixels.  With shift
    0 and values below 255 lo == hi is the exact nearest-rank percentile."""
    p = int(permille)
    if not 0 <= p <= 1000:
        raise ValueError("permille must be in [0, 1000]")
    M = int(record["pixels"])
    if M == 0:
        return 0, 0
    r = p * (M - 1) // 1000
    b = int(np.searchsorted(np.cumsum(np.asarray(record["bins"], dtype=np.uint64)), r, side="right"))
    shift, mn, mx = int(record["shift"]), int(record["min"]), int(record["max"])
    return max(mn, b << shift), (mx if b == 255 else min(mx, ((b + 1) << shift) - 1))


def _current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Context:
    """`device` >= 0 binds a GPU; device=None creates a host-only context (scene building
    and camera only -- every render entry then fails with RM_E_NO_DEVICE: no CPU path)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self.device = -1 if device is None else int(device)
        rc = N.lib().rm_create(self.device, C.byref(self._h))
        if rc != N.RM_OK:
            raise N.RmError(rc, "rm_create(device=%d) failed: no usable HIP device" % self.device)

    def close(self):
        if self._h:
            N.lib().rm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- options (never change results) -------------------------------------------
    def set_option(self, key, value):
        N.check(self._h, N.lib().rm_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        N.check(self._h, N.lib().rm_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    @contextlib.contextmanager
    def _exact(self, exact):
        """Option `exact` = 1 for the length of one call (the keyword `exact` of the point, field and mesh queries): the
        value the option had comes back afterwards, also when the call raises.  exact=False leaves the option as it is."""
        if not exact:
            yield
            return
        before = self.get_option("exact")
        self.set_option("exact", 1)
        try:
            yield
        finally:
            self.set_option("exact", before)

    def exact_tree(self):
        """What an exact query of the active scene walks (rm_debug_exact_tree; no device needed): dict(mode = 0 every object,
        1 the scene's BVH, 2 an exact tree of its own -- built now if it is due --, nodes, leaves, depth of that tree)."""
        out = (C.c_int32 * 4)()
        N.check(self._h, N.lib().rm_debug_exact_tree(self._h, out))
        return dict(mode=out[0], nodes=out[1], leaves=out[2], depth=out[3])

    def launch_fill(self, asked):
        """Workgroups per CU a v2 launch brings when `blocks_per_cu` is `asked`: option `min_fill` and the hardware-queue
        count the context read from GPU_MAX_HW_QUEUES when it was made (rm_debug_launch_fill; no device needed)."""
        v = C.c_int32(0)
        N.check(self._h, N.lib().rm_debug_launch_fill(self._h, int(asked), C.byref(v)))
        return v.value

    def last_launch(self):
        """The last launch of the v2 wave loop: dict(workgroups, threads, lds_bytes) and the context's CU count `cus`
        (rm_debug_last_launch; zeros before the first such launch)."""
        out = (C.c_uint32 * 4)()
        N.check(self._h, N.lib().rm_debug_last_launch(self._h, out))
        return dict(workgroups=out[0], threads=out[1], lds_bytes=out[2], cus=out[3])

    def overlap_fill(self, asked, items):
        """Workgroups per CU a v2 launch brings for a frame of `items` work items when `blocks_per_cu` is `asked`: the floor
        of launch_fill and, where the items pay for it, what option `overlap_fill` adds (rm_debug_overlap_fill; no device needed)."""
        v = C.c_int32(0)
        N.check(self._h, N.lib().rm_debug_overlap_fill(self._h, int(asked), int(items), C.byref(v)))
        return v.value

    def step_box(self):
        """Section M of the v2 wave loop and the scene's step-box table (rm_debug_step_box; no device needed but for `last`):
        dict(last = the last v2 launch tested its in-round steps against the table, planned = a launch of the active scene
        would under the options as they stand, reason = why not (0 it would, 1 options or kind of scene, 2 no table, 3 no
        room in LDS), list_cap / list_cap_without = the hit-list capacity of that launch with and without the table,
        table_bytes)."""
        out = (C.c_int32 * 6)()
        N.check(self._h, N.lib().rm_debug_step_box(self._h, out))
        return dict(last=bool(out[0]), planned=bool(out[1]), reason=out[2], list_cap=out[3], list_cap_without=out[4], table_bytes=out[5])

    def cell_tab(self):
        """Sections B and M of the v2 wave loop and the scene's cell table (rm_debug_cell_tab; no device needed but for
        `last`): dict(last = the last v2 launch read its candidates from the table, planned = a launch of the active scene
        would under the options as they stand, reason = why not (0 it would, 1 options, kind of scene or no step-box table
        in the launch, 2 no table, 3 no room in LDS), list_cap / list_cap_without, table_bytes, per_cu = workgroups of that
        launch a CU holds, scene_bytes / scene_bytes_without = what the launch stages, cells, records, leaf_sets)."""
        out = (C.c_int32 * 12)()
        N.check(self._h, N.lib().rm_debug_cell_tab(self._h, out))
        return dict(last=bool(out[0]), planned=bool(out[1]), reason=out[2], list_cap=out[3], list_cap_without=out[4], table_bytes=out[5],
                    per_cu=out[6], scene_bytes=out[7], scene_bytes_without=out[8], cells=out[9], records=out[10], leaf_sets=out[11])

    def runner_up(self):
        """Section M's runner-up test (rm_debug_runner_up; no device needed but for `last`): dict(last = the last v2 launch
        bounded the runner-up sphere of an in-round step by its own distance, planned = a launch of the active scene would
        under the options as they stand, reason = why not (0 it would, 1 option `runner_up` is 0, 2 the launch does not
        take the cell table, 3 the spheres do not share one radius))."""
        out = (C.c_int32 * 4)()
        N.check(self._h, N.lib().rm_debug_runner_up(self._h, out))
        return dict(last=bool(out[0]), planned=bool(out[1]), reason=out[2])

    @staticmethod
    def scan_keys(keys, rf=0.5):
        """The three-key update of the one-radius scan over a list of uint32 keys, from the kernel's own text on the host
        (rm_debug_scan_keys; no context state, no device): (the three smallest keys in order, 0xFFFFFFFF where there are
        fewer; the third key's lower bound for radius rf, +inf when fewer than three keys came; that bound as section M
        reads it, after its trip through the upper half of a word)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
        out = (C.c_uint32 * 3)()
        lb3, carried = C.c_float(0.0), C.c_float(0.0)
        N.check(None, N.lib().rm_debug_scan_keys(_ptr(k) if k.size else None, int(k.size), float(rf), out, C.byref(lb3), C.byref(carried)))
        return [int(out[0]), int(out[1]), int(out[2])], lb3.value, carried.value

    def rect_cull(self, rot, origin, width, height):
        """The leaf rectangles of the v2 bundle cull for a camera (rot[9], origin[3]: rm_camera_from_angles) and a full
        frame (rm_debug_rect_cull; no device needed but for `last`): dict(last = the last v2 launch culled by rectangles,
        planned = a launch of the active scene with this camera would, reason = why not (0 it would, 1 options or kind
        of scene, 2 too many leaves, 3 the camera or the frame), leaves, max_leaves)."""
        r = np.ascontiguousarray(rot, dtype=np.float32).reshape(9)
        o = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
        out = (C.c_int32 * 5)()
        N.check(self._h, N.lib().rm_debug_rect_cull(self._h, _ptr(r), _ptr(o), int(width), int(height), out))
        return dict(last=bool(out[0]), planned=bool(out[1]), reason=out[2], leaves=out[3], max_leaves=out[4])

    def leaf_rects(self, rot, origin, width, height):
        """The table of leaf screen rectangles such a launch fills, from the kernel's own text on the host
        (rm_debug_leaf_rects; no device needed): (rects uint16 [n, 4] = inclusive x_lo, x_hi, y_lo, y_hi; nodes int32 [n] =
        each leaf's index in the scene's BVH table).  n = 0: the launch would take the plane cull."""
        r = np.ascontiguousarray(rot, dtype=np.float32).reshape(9)
        o = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
        n = C.c_int64(0)
        N.check(self._h, N.lib().rm_debug_leaf_rects(self._h, _ptr(r), _ptr(o), int(width), int(height), None, None, 0, C.byref(n)))
        rects = np.zeros((max(1, n.value), 4), np.uint16)
        nodes = np.zeros(max(1, n.value), np.int32)
        N.check(self._h, N.lib().rm_debug_leaf_rects(self._h, _ptr(r), _ptr(o), int(width), int(height), _ptr(rects), _ptr(nodes),
                                                     n.value, C.byref(n)))
        return rects[:n.value], nodes[:n.value]

    # ---- scene ----------------------------------------------------------------------
    def scene_from_preset(self, index, accel):
        N.check(self._h, N.lib().rm_scene_from_preset(self._h, int(index), int(accel)))

    def scene_from_spheres(self, centers, radii, accel):
        c = np.ascontiguousarray(centers, dtype=np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
        if len(c) != len(r):
            raise ValueError("centers and radii differ in length")
        N.check(self._h, N.lib().rm_scene_from_spheres(self._h, _ptr(c), _ptr(r), len(r), int(accel)))

    def scene_from_prims(self, prims, accel):
        """prims: iterable of (type, world_to_local[16], params[<=3]); type 0 sphere, 1 box, 2 torus."""
        prims = list(prims)
        arr = (N.rm_prim * max(1, len(prims)))()
        for i, (t, m, par) in enumerate(prims):
            arr[i].type = int(t)
            for k in range(16):
                arr[i].world_to_local[k] = float(m[k])
            for k in range(3):
                arr[i].params[k] = float(par[k]) if k < len(par) else 0.0
        N.check(self._h, N.lib().rm_scene_from_prims(self._h, arr, len(prims), int(accel)))

    def scene_from_nodes(self, nodes, roots, accel):
        """SDF expression forest (rm_scene_from_nodes): nodes = iterable of
        (type, child_a, child_b, world_to_local[16] | None, params[<=6]); roots = Scene.objects."""
        nodes = list(nodes)
        arr = (N.rm_node * max(1, len(nodes)))()
        for i, (t, a, b, m, par) in enumerate(nodes):
            arr[i].type, arr[i].child_a, arr[i].child_b = int(t), int(a), int(b)
            for k in range(16):
                arr[i].world_to_local[k] = 0.0 if m is None else float(m[k])
            for k in range(6):
                arr[i].params[k] = float(par[k]) if k < len(par) else 0.0
        r = np.ascontiguousarray(roots, dtype=np.int32)
        N.check(self._h, N.lib().rm_scene_from_nodes(self._h, arr, len(nodes), _ptr(r), len(r), int(accel)))

    def edit_spheres(self, edits):
        """Edits the active sphere scene in place (rm_scene_edit_spheres; the rule is in include/rm_raymarch.h).  edits: a
        sequence of (op, index) for "remove" and (op, index, centre[3], radius) for "set" / "insert"; op a name of
        N.EDIT_OPS or an rm_edit_op value; or a ready array of N.rm_sphere_edit.  Indices are object indices at the moment
        each edit applies.  All or nothing."""
        arr, n = self._edit_array(edits)
        N.check(self._h, N.lib().rm_scene_edit_spheres(self._h, arr, n))

    @staticmethod
    def _edit_array(edits):
        if isinstance(edits, C.Array) and edits._type_ is N.rm_sphere_edit:
            return edits, len(edits)
        edits = list(edits)
        n = len(edits)
        arr = (N.rm_sphere_edit * max(1, n))()
        for k, e in enumerate(edits):
            arr[k].op = N.EDIT_OPS[e[0]] if isinstance(e[0], str) else int(e[0])
            arr[k].index = int(e[1])
            if len(e) > 2:
                arr[k].center[:] = [float(v) for v in np.asarray(e[2], np.float32).reshape(3)]
                arr[k].radius = float(e[3])
        return arr, n

    def edit_balls(self, edits):
        """The balls of an edit list (rm_scene_edit_balls; host-only): for every sphere version the edits remove or add, its
        centre and radius, in edit order -- what rm_scene_tiles_update_device needs to know of the edit.  Call it BEFORE
        edit_spheres with the same list; it changes nothing.  Returns a numpy record array of N.BALL_DTYPE."""
        arr, n = self._edit_array(edits)
        count = C.c_int32(0)
        out = np.zeros(2 * n, N.BALL_DTYPE)
        N.check(self._h, N.lib().rm_scene_edit_balls(self._h, arr, n, out.ctypes.data_as(C.POINTER(N.rm_ball)) if n else None, 2 * n, C.byref(count)))
        return out[:count.value]

    def scene_table(self, name, from_device=True):
        """One table of the active scene (rm_debug_scene_table) as a numpy array of N.SCENE_TABLES[name] (records as
        bytes): the device copy, or with from_device=False the host builder's (the only form a host-only context has)."""
        size = C.c_int64(0)
        key = name.encode()
        N.check(self._h, N.lib().rm_debug_scene_table(self._h, key, int(bool(from_device)), None, 0, C.byref(size)))
        out = np.zeros(size.value, np.uint8)
        N.check(self._h, N.lib().rm_debug_scene_table(self._h, key, int(bool(from_device)), _ptr(out), out.size, C.byref(size)))
        return out.view(N.SCENE_TABLES.get(name, "u1"))

    def selftest_hypot64(self, xyz, on_device=True):
        """Math.hypot of float64 triples [n, 3] as the host scene builder (on_device=False) or the device builder
        evaluates it (rm_selftest_hypot64)."""
        a = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(len(a), np.float64)
        N.check(self._h, N.lib().rm_selftest_hypot64(self._h, _ptr(a), len(a), int(bool(on_device)), _ptr(out)))
        return out

    def scene_set_time(self, time):
        """Scene.updateTime(time) for scene_distance (renders take the job's time)."""
        N.check(self._h, N.lib().rm_scene_set_time(self._h, float(time)))

    def selftest_jsmath(self, fn, a, b=None):
        """Math.sin/cos/atan2/asin/log/pow/round/atan (fn 0..7) as the device evaluates them."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        out = np.zeros_like(a)
        N.check(self._h, N.lib().rm_selftest_jsmath(self._h, int(fn), _ptr(a), _ptr(b), a.size, _ptr(out)))
        return out

    def scene_info(self):
        info = N.rm_scene_info()
        N.check(self._h, N.lib().rm_scene_get_info(self._h, C.byref(info)))
        d = {k: getattr(info, k) for k, _ in info._fields_ if k not in ("root_min", "root_max", "reserved")}
        d["root_min"] = [float(v) for v in info.root_min]
        d["root_max"] = [float(v) for v in info.root_max]
        # expression forests: what the interpreter's program needs (0 for the other scene kinds)
        d["prog_slots"], d["prog_vals"], d["prog_instructions"] = info.program & 0xFF, (info.program >> 8) & 0xFF, info.program >> 16
        return d

    def scene_distance(self, points):
        """Scene.getDistance for a batch of points -> (dist float64[n], count uint32[n])."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        dist = np.zeros(len(p), np.float64)
        cnt = np.zeros(len(p), np.uint32)
        N.check(self._h, N.lib().rm_scene_distance(self._h, _ptr(p), len(p), _ptr(dist), _ptr(cnt)))
        return dist, cnt

    def wave_distance(self, points):
        """scene_distance through the v2 wave loop's distance function (rm_debug_wave_distance; BVH sphere scenes)."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        dist = np.zeros(len(p), np.float64)
        cnt = np.zeros(len(p), np.uint32)
        N.check(self._h, N.lib().rm_debug_wave_distance(self._h, _ptr(p), len(p), _ptr(dist), _ptr(cnt)))
        return dist, cnt

    def ray_march(self, origins, directions, algorithm="sphere-tracer", normal=True, time=0.0, overshoot=None, step=None):
        """Raymarcher.rayMarch (+ getNormal at hits when `normal`) for caller-supplied rays through the active scene
        (rm_ray_march).  origins, directions: float32 [n, 3] (directions are used as given, not normalised).  Returns
        (t float64[n], iters uint32[n], sdf_calls uint32[n], normal float32[n, 3]); counts are exact (the reference's
        Uint16Array buffers hold them mod 65536).  numpy input -> the host entry (synchronous); torch CUDA tensors ->
        rm_ray_march_device on torch's current stream, outputs allocated on the same device -- there iters and sdf_calls are
        int32 tensors holding the u32 bits (torch's uint32 tensors support few operations; the counts stay below 2^31).  `algorithm`: a name of
        ALGORITHMS or an rm_algorithm value; overshoot / step None mirror JS `undefined` (1.2 / 0.1)."""
        return self._rays(False, origins, directions, algorithm, normal, time, overshoot, step)

    def pick(self, origins, directions, algorithm="sphere-tracer", normal=True, time=0.0, overshoot=None, step=None):
        """ray_march plus the object each ray hit (rm_ray_pick): returns (t, iters, sdf_calls, normal, object), the first
        four bit-identical to ray_march's, object int32[n] an index into the scene's objects in the order the scene was
        built in (-1: none; the rule is in include/rm_raymarch.h).  numpy input -> the host entry; torch CUDA tensors ->
        rm_ray_pick_device on torch's current stream (object an int32 tensor on the same device)."""
        return self._rays(True, origins, directions, algorithm, normal, time, overshoot, step)

    @staticmethod
    def _query(algorithm, normal, time, overshoot, step):
        """The rm_ray_query of a call; overshoot / step None -> NaN (JS `undefined`)."""
        q = N.rm_ray_query()
        q.algorithm = (N.lib().rm_algorithm_from_string(algorithm.encode()) if isinstance(algorithm, str) else int(algorithm))
        q.normal = 1 if normal else 0
        q.time = float(time)
        q.overshoot_factor = float(overshoot) if overshoot is not None else float("nan")
        q.step_size = float(step) if step is not None else float("nan")
        return q

    def _ray_input(self, origins, directions):
        """(on_device, origins, directions, n) of a ray query's input: contiguous float32 CUDA tensors of this context's device
        as they are, anything else as float32 [n, 3] numpy arrays."""
        if _is_torch(origins) or _is_torch(directions):
            import torch
            if not (_is_torch(origins) and _is_torch(directions) and origins.is_cuda and directions.is_cuda):
                raise ValueError("origins and directions must both be CUDA tensors (or both numpy arrays)")
            self._same_device(dict(origins=origins, directions=directions))
            for name, b in (("origins", origins), ("directions", directions)):
                if b.dtype != torch.float32 or not b.is_contiguous() or b.numel() % 3:
                    raise ValueError("%s must be a contiguous float32 tensor of [n, 3]" % name)
            if directions.numel() != origins.numel():
                raise ValueError("origins and directions differ in length")
            return True, origins, directions, origins.numel() // 3
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        if len(o) != len(d):
            raise ValueError("origins and directions differ in length")
        return False, o, d, len(o)

    def _frame_rays(self, width, height, pitch, yaw, y_start, y_end, device):
        """The camera rays of rows [y_start, y_end) (y_end None: height) with the origin repeated per ray -> (origins, directions,
        rows): float32 [n, 3] numpy arrays, or with `device` CUDA tensors of this context's device, and the number of rows."""
        if y_end is None:
            y_end = height
        org, dirs = camera_rays(width, height, pitch, yaw, y_start, y_end)
        o = np.ascontiguousarray(np.broadcast_to(org, dirs.shape))
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            o, dirs = torch.from_numpy(o).to(dev), torch.from_numpy(dirs).to(dev)
        return o, dirs, y_end - y_start

    def _rays(self, pick, origins, directions, algorithm, normal, time, overshoot, step):
        """ray_march (pick False) or pick (True)."""
        q = self._query(algorithm, normal, time, overshoot, step)
        on_dev, o, d, n = self._ray_input(origins, directions)
        L = N.lib()
        if on_dev:
            import torch
            # (the u32 counts as int32 tensors: same bits; counts stay < 2^31)
            out = [torch.empty(n, dtype=torch.float64, device=o.device), torch.empty(n, dtype=torch.int32, device=o.device),
                   torch.empty(n, dtype=torch.int32, device=o.device), torch.empty((n, 3), dtype=torch.float32, device=o.device)]
            if pick:
                out.append(torch.empty(n, dtype=torch.int32, device=o.device))
            entry = L.rm_ray_pick_device if pick else L.rm_ray_march_device
            N.check(self._h, entry(self._h, C.byref(q), n, _ptr(o), _ptr(d), *[_ptr(b) for b in out], _current_stream_ptr()))
            return tuple(out)
        out = [np.zeros(n, np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 3), np.float32)]
        if pick:
            out.append(np.zeros(n, np.int32))
        entry = L.rm_ray_pick if pick else L.rm_ray_march
        N.check(self._h, entry(self._h, C.byref(q), n, _ptr(o), _ptr(d), *[_ptr(b) for b in out]))
        return tuple(out)

    def object_ids(self, width, height, pitch=0.0, yaw=0.0, y_start=0, y_end=None, algorithm="sphere-tracer", time=0.0,
                   device=False):
        """The object under every pixel of rows [y_start, y_end) of a width x height frame of the active scene (a selection
        mask or outline without a render kernel): the frame's camera rays (camera_rays) picked without normals ->
        int32[(y_end - y_start) * width], tile-local rows, row-major, -1 where no object was hit.  device=True: the rays go
        to rm_ray_pick_device as CUDA tensors of this context's device and the result is one."""
        o, dirs, _ = self._frame_rays(width, height, pitch, yaw, y_start, y_end, device)
        return self.pick(o, dirs, algorithm, normal=False, time=time)[4]

    def light(self, origins, directions, light_dir=None, bias=0.02, ao_samples=5, ao_step=0.05, ao_strength=1.0,
              algorithm="sphere-tracer", time=0.0, overshoot=None, step=None):
        """ray_march with normals plus two light terms at each hit, in one launch (rm_ray_light; the rule is in
        include/rm_raymarch.h): returns (t, iters, sdf_calls, normal, lit, ao, iters2, sdf_calls2), the first four
        bit-identical to ray_march(..., normal=True).  lit float32[n]: 0 where the surface faces away from `light_dir` or a
        shadow ray from f32(p + n * bias) towards it, marched by the same marcher, hits something; else 1.  ao float32[n]:
        1 - ao_strength * sum_k (k * ao_step - getDistance(p + n * k * ao_step)) / 2^(k-1) over ao_samples (0 .. 8) samples,
        clamped to [0, 1].  iters2 / sdf_calls2: the shadow ray's iterations, and its SDF calls plus the samples'.  Misses
        give lit = ao = 1.  light_dir None: phong_light(), the direction the Phong shader uses; it is taken as given, not
        normalised.  The default bias must exceed the marchers' hit threshold of 0.001, or every shadow ray hits its own
        surface at once; 0.02 is a choice that clears it on the presets, not a measured optimum.  numpy input -> the host
        entry; torch CUDA tensors -> rm_ray_light_device on torch's current stream (counts as int32 tensors, as ray_march)."""
        q = self._query(algorithm, True, time, overshoot, step)
        lt = N.rm_light()
        lt.dir[:] = [float(v) for v in (phong_light() if light_dir is None else np.asarray(light_dir, np.float32).reshape(3))]
        lt.ao_samples = int(ao_samples)
        lt.bias, lt.ao_step, lt.ao_strength = float(bias), float(ao_step), float(ao_strength)
        on_dev, o, d, n = self._ray_input(origins, directions)
        if on_dev:
            import torch
            dev = o.device
            out = (torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev),
                   torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
            N.check(self._h, N.lib().rm_ray_light_device(self._h, C.byref(q), C.byref(lt), n, _ptr(o), _ptr(d), *[_ptr(b) for b in out],
                                                         _current_stream_ptr()))
            return out
        out = (np.zeros(n, np.float64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 3), np.float32),
               np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
        N.check(self._h, N.lib().rm_ray_light(self._h, C.byref(q), C.byref(lt), n, _ptr(o), _ptr(d), *[_ptr(b) for b in out]))
        return out

    def light_frame(self, width, height, pitch=0.0, yaw=0.0, y_start=0, y_end=None, light_dir=None, bias=0.02, ao_samples=5,
                    ao_step=0.05, ao_strength=1.0, algorithm="sphere-tracer", time=0.0, device=False):
        """The light terms under every pixel of rows [y_start, y_end) of a width x height frame of the active scene: the
        frame's camera rays (camera_rays) through `light` -> (lit, ao), float32[(y_end - y_start) * width] each, tile-local
        rows, row-major: what shade_lit takes beside the frame's depth and normal buffers.  device=True: the rays go to
        rm_ray_light_device as CUDA tensors of this context's device and the results are tensors."""
        o, dirs, _ = self._frame_rays(width, height, pitch, yaw, y_start, y_end, device)
        out = self.light(o, dirs, light_dir=light_dir, bias=bias, ao_samples=ao_samples, ao_step=ao_step, ao_strength=ao_strength,
                         algorithm=algorithm, time=time)
        return out[4], out[5]

    def walk(self, origins, directions, algorithm="sphere-tracer", time=0.0, overshoot=None, step=None, trace=False, cap=200):
        """How the marcher walks each ray, in one launch (rm_ray_walk; the rule is in include/rm_raymarch.h).  Returns `walks`,
        one record of WALK_DTYPE per ray (t as ray_march returns it, min_dist / t_min: the closest evaluation and where,
        skipped / skips: what the acceleration structure skipped, evals, sdf_calls, end: an RM_END_* value, WALK_ENDS names
        them), or with `trace` (walks, steps): steps[n, cap] of STEP_DTYPE holds the first min(cap, evals + skips) records of
        each ray -- one per distance evaluation (kind 0: t, the distance, the primitives counted) and per skip (kind 1: t
        before it, its length) -- and zeros behind them.  No walk produces more than 200 records.  numpy input -> the host
        entry and structured arrays; torch CUDA tensors -> rm_ray_walk_device on torch's current stream and uint8 tensors
        [n, 48] and [n, cap, 24] holding the same records (`.cpu().numpy().view(...)` with the dtypes gives the fields)."""
        q = self._query(algorithm, False, time, overshoot, step)
        cap = int(cap)
        on_dev, o, d, n = self._ray_input(origins, directions)
        if on_dev:
            import torch
            walks = torch.empty((n, 48), dtype=torch.uint8, device=o.device)
            steps = torch.zeros((n, max(cap, 0), 24), dtype=torch.uint8, device=o.device) if trace else None
            N.check(self._h, N.lib().rm_ray_walk_device(self._h, C.byref(q), n, _ptr(o), _ptr(d), cap if trace else 0, _ptr(walks), _ptr(steps),
                                                        _current_stream_ptr()))
            return (walks, steps) if trace else walks
        walks = np.zeros(n, N.WALK_DTYPE)
        steps = np.zeros((n, max(cap, 0)), N.STEP_DTYPE) if trace else None
        N.check(self._h, N.lib().rm_ray_walk(self._h, C.byref(q), n, _ptr(o), _ptr(d), cap if trace else 0, _ptr(walks), _ptr(steps)))
        return (walks, steps) if trace else walks

    def walk_frame(self, width, height, pitch=0.0, yaw=0.0, y_start=0, y_end=None, algorithm="sphere-tracer", time=0.0,
                   overshoot=None, step=None, device=False):
        """The walk summaries under every pixel of rows [y_start, y_end) of a width x height frame of the active scene: the
        frame's camera rays (camera_rays) through `walk` -> WALK_DTYPE[rows, width], tile-local rows (an end-reason map is
        its "end" field, a skipped-distance map its "skipped").  device=True: the rays go to rm_ray_walk_device as CUDA
        tensors of this context's device and the result is a uint8 tensor [rows, width, 48]."""
        o, dirs, rows = self._frame_rays(width, height, pitch, yaw, y_start, y_end, device)
        walks = self.walk(o, dirs, algorithm=algorithm, time=time, overshoot=overshoot, step=step)
        return walks.reshape(rows, width, 48) if device else walks.reshape(rows, width)

    def trace_pixel(self, width, height, x, y, pitch=0.0, yaw=0.0, algorithm="sphere-tracer", time=0.0, overshoot=None, step=None):
        """The whole walk of the ray through pixel (x, y) of a width x height frame of the active scene -> (walk, steps):
        the pixel's summary record and its step records, trimmed to the evals + skips the walk produced."""
        o, dirs, _ = self._frame_rays(width, height, pitch, yaw, int(y), int(y) + 1, False)
        walks, steps = self.walk(o[int(x)].reshape(1, 3), dirs[int(x)].reshape(1, 3), algorithm=algorithm, time=time, overshoot=overshoot,
                                 step=step, trace=True, cap=N.RM_WALK_MAX_STEPS)
        return walks[0], steps[0, :int(walks[0]["evals"]) + int(walks[0]["skips"])]

    def shade_lit(self, depth, normal, lit, ao, rgba, width=0, rows=0, n_frames=1):
        """The Phong shade with the light terms of `light` / `light_frame` (rm_shade_lit_device / rm_shade_lit):
        I = min((0.1 + diffuse * lit + specular * lit) * ao, 1); lit = ao = 1 gives the "phong" shader's bytes.  depth,
        normal: a render's G-buffers; lit, ao: float32, one per pixel; n_frames frames of width x rows pixels, frame after
        frame in every buffer.  torch CUDA tensors -> the device entry on torch's current stream; numpy arrays -> the host
        entry (synchronous)."""
        n = int(n_frames)
        npx = max(0, int(width)) * max(0, int(rows)) * max(0, n)
        on_dev = _check_buffers(npx, dict(depth=depth, normal=normal, rgba=rgba))
        for name, b in (("lit", lit), ("ao", ao)):
            if b is None:
                continue
            dev, contiguous, _, nbytes, _ = _describe(name, b)
            if str(b.dtype) not in ("float32", "torch.float32") or not contiguous or nbytes < 4 * npx:
                raise ValueError("%s must be a contiguous float32 buffer of one element per pixel" % name)
            if dev != on_dev and (depth is not None or normal is not None or rgba is not None):
                raise ValueError(_MIXED)
        self._same_device(dict(depth=depth, normal=normal, lit=lit, ao=ao, rgba=rgba))
        self._both("rm_shade_lit", on_dev, int(width), int(rows), n, _ptr(depth), _ptr(normal), _ptr(lit), _ptr(ao), _ptr(rgba))
        return rgba

    def scene_object(self, index):
        """Object `index` of the active scene (rm_scene_object) as (nodes, root): nodes is a list of
        (type, child_a, child_b, world_to_local float32[16], params float64[6]) in the format OracleScene.nodes() and
        Scene.loadNodes use, operands before their user, the object's root last (root = len(nodes) - 1)."""
        n = C.c_int32(0)
        N.check(self._h, N.lib().rm_scene_object(self._h, int(index), None, 0, C.byref(n)))
        arr = (N.rm_node * max(1, n.value))()
        N.check(self._h, N.lib().rm_scene_object(self._h, int(index), arr, n.value, C.byref(n)))
        return [(int(e.type), int(e.child_a), int(e.child_b), np.array(e.world_to_local, np.float32), np.array(e.params, np.float64))
                for e in arr[:n.value]]

    # ---- render ---------------------------------------------------------------------
    def _attach_diag(self, diag):
        """rm_render_attach_diagnostics for the render call that follows: `diag` is a CUDA tensor of 32 bytes that
        receives (total_sdf, total_iters, max_sdf | min_sdf << 32, pad) of the pixels that call renders (decode_acc)."""
        if diag is None:
            return
        if _bytes_on(True, diag) < 32:
            raise ValueError("diag must be a contiguous CUDA tensor of 32 bytes")
        self._same_device(dict(diag=diag))
        N.check(self._h, N.lib().rm_render_attach_diagnostics(self._h, _ptr(diag)))

    def render_tile(self, job, depth, normal, sdf, iters, rgba=None, shader=0, diag=None):
        """Host numpy buffers -> rm_render_tile (+ rm_shade when rgba is given); torch CUDA
        tensors -> rm_render_tile_device on torch's current stream (fused shade; `diag`: fused diagnostics)."""
        npx = max(0, job.y_end - job.y_start) * max(0, job.width)
        bufs = dict(depth=depth, normal=normal, sdf=sdf, iters=iters, rgba=rgba)
        if _check_buffers(npx, bufs) or (diag is not None and all(b is None for b in bufs.values())):
            self._same_device(bufs)
            self._attach_diag(diag)
            N.check(self._h, N.lib().rm_render_tile_device(
                self._h, C.byref(job), int(shader), _ptr(depth), _ptr(normal), _ptr(sdf), _ptr(iters),
                _ptr(rgba), _current_stream_ptr()))
            return
        if diag is not None:
            raise ValueError("fused diagnostics need device buffers")
        if depth is None or normal is None or sdf is None or iters is None:
            raise ValueError("the host entry point needs all four G-buffers")
        N.check(self._h, N.lib().rm_render_tile(self._h, C.byref(job), _ptr(depth), _ptr(normal),
                                                 _ptr(sdf), _ptr(iters)))
        if rgba is not None:
            rows = max(0, job.y_end - job.y_start)
            self.shade(shader, job.width, rows, depth, normal, sdf, iters, rgba)

    def render_frames(self, job, views, depth, normal, sdf, iters, rgba=None, shader=0, diag=None):
        """len(views) frames of one scene in one launch (rm_render_frames_device) on torch's current stream.  `job` gives what
        the frames share (its own camera and time are ignored); `views` is a sequence of (pitch, yaw, time) or an (n, 3)
        float64 array (sweep_views).  depth / normal / sdf / iters / rgba: CUDA tensors that hold the n frames one behind the
        other (frame k at pixel k * width * rows), or None; `diag`: None or a CUDA tensor of 32 * n bytes that receives one
        accumulator per frame (decode_accs)."""
        v = np.ascontiguousarray(views, dtype=np.float64).reshape(-1, 3)
        n = len(v)
        npx = max(0, job.y_end - job.y_start) * max(0, job.width)
        bufs = dict(depth=depth, normal=normal, sdf=sdf, iters=iters, rgba=rgba)
        _check_buffers(npx * n, bufs, need_device=True)
        self._same_device(bufs)
        if diag is not None:
            if _bytes_on(True, diag) < 32 * n:
                raise ValueError("diag must be a contiguous CUDA tensor of 32 bytes per view")
            self._same_device(dict(diag=diag))
        N.check(self._h, N.lib().rm_render_frames_device(
            self._h, C.byref(job), int(shader), _ptr(v), n, _ptr(depth), _ptr(normal), _ptr(sdf), _ptr(iters), _ptr(rgba),
            _ptr(diag), _current_stream_ptr() if self.device >= 0 else None))  # (a host-only context: RM_E_NO_DEVICE from the library)

    # ---- two renders of a view: difference image and statistics ------------------------
    def compare_frames(self, a, b, rgba=None, map="sdf", gain=5, stats=None, width=0, rows=0, n_frames=1):
        """B against A for n_frames frames of width x rows pixels (rm_compare_frames_device / rm_compare_frames).  a, b:
        (depth, normal, sdf, iters), the n frames one behind the other as render_frames writes them; a pair may be None on
        both sides (the fields derived from it are 0).  `map`: a name of COMPARE_MAPS ("none", "sdf", "iters", "depth",
        "normal", "surface") or an rm_compare_map value -- the difference image written to `rgba` (4 bytes per pixel; None
        only with "none"); `gain` 1 .. 255.  `stats`: None, or a buffer of 128 * n_frames bytes for one rm_compare_stats per
        frame (decode_compare_stats).  torch CUDA tensors -> the device entry on torch's current stream (asynchronous); numpy
        arrays -> the host entry (synchronous).  Neither rgba nor stats needs a pre-clear."""
        if a is None or b is None:
            a = b = None
            sides = [None, None]
        else:
            if len(a) != 4 or len(b) != 4:
                raise ValueError("a and b are (depth, normal, sdf, iters)")
            sides = [N.rm_frame_set(*[getattr(_ptr(x), "value", None) for x in side]) for side in (a, b)]
        m = _compare_map(map)
        n = int(n_frames)
        npx = max(0, int(width)) * max(0, int(rows)) * max(0, n)
        bufs = {}
        for side, tag in ((a, "_a"), (b, "_b")):
            for name, x in zip(("depth", "normal", "sdf", "iters"), side or ()):
                bufs[name + tag] = x
        on_dev = _check_pixel_sets(npx, bufs, rgba, stats, n)
        self._same_device(dict(bufs, rgba=rgba, stats=stats))
        refs = [None if x is None else C.byref(x) for x in sides]
        self._both("rm_compare_frames", on_dev, int(width), int(rows), n, refs[0], refs[1], m, int(gain), _ptr(rgba), _ptr(stats))

    @staticmethod
    def decode_compare_stats(buf):
        """One dict per 128-byte rm_compare_stats record of `buf` (a CUDA tensor or a numpy array, compare_frames' stats)."""
        raw = buf.cpu().contiguous().view(-1).numpy() if _is_torch(buf) else np.ascontiguousarray(buf).reshape(-1)
        raw = raw.view(np.uint8)
        out = []
        for k in range(raw.size // 128):
            rec = N.rm_compare_stats.from_buffer_copy(raw[128 * k:128 * (k + 1)].tobytes())
            out.append({name: int(getattr(rec, name)) for name, _ in N.rm_compare_stats._fields_})
        return out

    def compare(self, job_a, job_b, views=None, shader=None, map="sdf", gain=5):
        """Renders job_a and job_b into buffers of its own and compares them, B against A: returns (stats, rgba) -- a list of
        one dict per frame and the difference image as a CUDA uint8 tensor [n, rows, width, 4].  `views` (as render_frames
        takes them): that many frames per job through render_frames, else one frame through render_tile with each job's own
        camera.  The jobs must agree in width, height, rows and scene; they may differ in algorithm, acceleration
        structure, overshoot and step size.  `shader`: None, or the shading model the two renders also run -- the result is
        then (stats, rgba, shaded_a, shaded_b)."""
        import torch
        for f in ("width", "height", "y_start", "y_end", "scene_preset_index"):
            if getattr(job_a, f) != getattr(job_b, f):
                raise ValueError("the jobs differ in %s" % f)
        W, rows = max(0, job_a.width), max(0, job_a.y_end - job_a.y_start)
        n = 1 if views is None else len(np.ascontiguousarray(views, dtype=np.float64).reshape(-1, 3))
        dev, total = torch.device("cuda", self.device), W * rows * n
        sets, shaded = [], []
        for job in (job_a, job_b):
            g = (torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(3 * total, dtype=torch.uint8, device=dev),
                 torch.empty(total, dtype=torch.int16, device=dev), torch.empty(total, dtype=torch.int16, device=dev))
            img = None if shader is None else torch.empty(4 * total, dtype=torch.uint8, device=dev)
            if views is None:
                self.render_tile(job, *g, rgba=img, shader=shader or 0)
            else:
                self.render_frames(job, views, *g, rgba=img, shader=shader or 0)
            sets.append(g)
            shaded.append(img)
        m = _compare_map(map)
        rgba = None if m < 0 else torch.empty(4 * total, dtype=torch.uint8, device=dev)
        stats = torch.empty(128 * n, dtype=torch.uint8, device=dev)
        self.compare_frames(sets[0], sets[1], rgba=rgba, map=m, gain=gain, stats=stats, width=W, rows=rows, n_frames=n)
        out = (self.decode_compare_stats(stats), None if rgba is None else rgba.view(n, rows, W, 4))
        return out if shader is None else out + tuple(x.view(n, rows, W, 4) for x in shaded)

    # ---- counter distributions per frame: histograms, percentiles, ranged heatmaps --------
    def counter_hist(self, sdf, iters, normal=None, mask="all", bin_shift=0, percentiles=(0, 1000), hist=None, width=0, rows=0,
                     n_frames=1):
        """The histogram of each counter of each of n_frames frames of width x rows pixels (rm_counter_hist_device /
        rm_counter_hist), the frames one behind the other as render_frames writes them.  sdf, iters: either may be None (its
        records are zero), not both.  `mask`: a name of HIST_MASKS ("all", "surface", "background") or an rm_hist_mask value;
        the last two need `normal`.  bin(v) = min(v >> bin_shift, 255); `percentiles`: the two permille values (lo, hi) behind
        range_lo and range_hi.  `hist`: a buffer of 2128 * n_frames bytes for one rm_frame_hist per frame (decode_hists), or
        None: one is allocated beside the counters.  Returns it.  torch CUDA tensors -> the device entry on torch's current
        stream (asynchronous); numpy arrays -> the host entry (synchronous).  hist needs no pre-clear."""
        m = N.HIST_MASKS[mask] if isinstance(mask, str) else int(mask)
        n = int(n_frames)
        npx = max(0, int(width)) * max(0, int(rows)) * max(0, n)
        bufs = dict(sdf=sdf, iters=iters, normal=normal)
        on_dev = _check_buffers(npx, bufs)
        if sdf is None and iters is None and normal is None:
            on_dev = None  # (no pixel buffer: the records decide the side)
        if hist is None:
            if on_dev:
                import torch
                some = next(b for b in bufs.values() if b is not None)
                hist = torch.empty(2128 * max(0, n), dtype=torch.uint8, device=some.device)
            else:
                hist = np.zeros(2128 * max(0, n), np.uint8)
                on_dev = False
        on_dev = _check_records("hist", hist, 2128, n, on_dev)
        self._same_device(dict(bufs, hist=hist))
        lo, hi = (int(x) for x in percentiles)
        self._both("rm_counter_hist", on_dev, int(width), int(rows), n, _ptr(sdf), _ptr(iters), _ptr(normal), m, int(bin_shift), lo, hi, _ptr(hist))
        return hist

    @staticmethod
    def decode_hists(buf):
        """One {"sdf": {...}, "iters": {...}} per 2128-byte rm_frame_hist record of `buf` (a CUDA tensor or a numpy array,
        counter_hist's hist): the fields of rm_counter_hist as ints, `bins` as a numpy uint32[256] array."""
        raw = buf.cpu().contiguous().view(-1).numpy() if _is_torch(buf) else np.ascontiguousarray(buf).reshape(-1)
        raw = raw.view(np.uint8)
        out = []
        for k in range(raw.size // 2128):
            rec = N.rm_frame_hist.from_buffer_copy(raw[2128 * k:2128 * (k + 1)].tobytes())
            frame = {}
            for name in ("sdf", "iters"):
                c = getattr(rec, name)
                d = {f: int(getattr(c, f)) for f, _ in N.rm_counter_hist._fields_ if f != "bins"}
                d["bins"] = np.frombuffer(bytes(c.bins), dtype=np.uint32).copy()
                frame[name] = d
            out.append(frame)
        return out

    def shade_ranged(self, counter, values, rgba, hist=None, lo=0, hi=0, width=0, rows=0, n_frames=1):
        """The heatmap of one counter scaled to a range (rm_shade_ranged_device / rm_shade_ranged): s = 0 up to lo, 255 from hi,
        (v - lo) * 255 // (hi - lo) between, coloured by the reference's red-green ramp; it never wraps.  `counter`: "sdf" / 0 or
        "iters" / 1 -- what `values` holds.  `hist`: None (every frame uses lo, hi) or counter_hist's records: frame k then takes
        range_lo, range_hi of its own record, read on the device -- no synchronisation is needed between the two calls.
        torch CUDA tensors -> the device entry on torch's current stream; numpy arrays -> the host entry (synchronous)."""
        c = {"sdf": 0, "iters": 1}[counter] if isinstance(counter, str) else int(counter)
        n = int(n_frames)
        npx = max(0, int(width)) * max(0, int(rows)) * max(0, n)
        bufs = dict(sdf=values, rgba=rgba)
        on_dev = _check_buffers(npx, bufs)
        if hist is not None:
            _check_records("hist", hist, 2128, n, on_dev if (values is not None or rgba is not None) else None)
        self._same_device(dict(bufs, hist=hist))
        self._both("rm_shade_ranged", on_dev, c, int(width), int(rows), n, _ptr(values), _ptr(hist), int(lo), int(hi), _ptr(rgba))
        return rgba

    # ---- field queries: distance slices and volumes sampled on the device ------------------
    def lattice_points(self, origin, du, dv, dw=None, shape=(1, 1)):
        """The points of a lattice (rm_lattice_points) as float32 [nw, nv, nu, 3]: point (i, j, k) is
        f32(origin + i * du + j * dv + k * dw), formed in binary64 with one rounding, exactly what `field` evaluates."""
        lat = make_lattice(origin, du, dv, dw, shape)
        out = np.zeros((lat.nw, lat.nv, lat.nu, 3), np.float32)
        rc = N.lib().rm_lattice_points(C.byref(lat), 0, out.size // 3, _ptr(out))
        if rc != N.RM_OK:
            raise N.RmError(rc, "rm_lattice_points")
        return out

    def field(self, origin, du, dv, dw=None, shape=(1, 1), time=0.0, dist32=False, count=True, device=False, exact=False):
        """Scene.getDistance at every point of a lattice the device forms itself (rm_scene_field; the rule is in
        include/rm_raymarch.h): point (i, j, k) = f32(origin + i * du + j * dv + k * dw), shape = (nu, nv) for a slice or
        (nu, nv, nw) for a volume.  Returns (dist, count) shaped [nw, nv, nu] -- [nv, nu] for a two-element shape --: dist
        float64, or float32 with `dist32` (half the traffic of a volume), count uint32 (the primitives each evaluation
        counted) or None without `count`.  The values are scene_distance's at lattice_points(...) with the scene at `time`;
        scene_set_time's value is left alone.  numpy results come through the host entry (synchronous); device=True returns
        torch CUDA tensors through rm_scene_field_device on torch's current stream (count an int32 tensor holding the u32
        bits, as ray_march's counts).  exact=True: the exact field (option `exact` for this call) -- min(10, min over ALL
        objects of Primitive.sdf), what an acceleration-None upload answers, whatever structure the scene has; count is then
        the evaluations made."""
        with self._exact(exact):
            return self._field(origin, du, dv, dw, shape, time, dist32, count, device)

    def _field(self, origin, du, dv, dw, shape, time, dist32, count, device):
        lat = make_lattice(origin, du, dv, dw, shape, time)
        full = (lat.nw, lat.nv, lat.nu)
        out_shape = full[1:] if len(tuple(shape)) == 2 else full
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            d = torch.empty(full, dtype=torch.float32 if dist32 else torch.float64, device=dev)
            c = torch.empty(full, dtype=torch.int32, device=dev) if count else None
            N.check(self._h, N.lib().rm_scene_field_device(self._h, C.byref(lat), None if dist32 else _ptr(d), _ptr(d) if dist32 else None,
                                                           _ptr(c), _current_stream_ptr()))
        else:
            d = np.zeros(full, np.float32 if dist32 else np.float64)
            c = np.zeros(full, np.uint32) if count else None
            N.check(self._h, N.lib().rm_scene_field(self._h, C.byref(lat), None if dist32 else _ptr(d), _ptr(d) if dist32 else None, _ptr(c)))
        return d.reshape(out_shape), (None if c is None else c.reshape(out_shape))

    def field_slice(self, axis="z", offset=0.0, half_extent=5.0, size=(256, 256), time=0.0, dist32=False, count=True, device=False, exact=False):
        """`field` of slice_lattice(axis, offset, half_extent, size): the axis-aligned plane through the scene, sampled at
        texel centres -> (dist, count) shaped [size[1], size[0]]."""
        origin, du, dv, shape = slice_lattice(axis, offset, half_extent, size)
        return self.field(origin, du, dv, shape=shape, time=time, dist32=dist32, count=count, device=device, exact=exact)

    @staticmethod
    def slice_lattice(axis="z", offset=0.0, half_extent=5.0, size=(256, 256)):
        """The module's slice_lattice: (origin, du, dv, shape) of an axis-aligned plane sampled at texel centres."""
        return slice_lattice(axis, offset, half_extent, size)

    def shade_field(self, values, rgba=None, map="distance", range=2.0, band=0.25, line=0.02, lo=0, hi=0):
        """The slice image of `field`'s results (rm_shade_field_device / rm_shade_field; the rule is in
        include/rm_raymarch.h).  map "distance": `values` float64 -- blue inside, orange outside, brighter with |d| up to
        `range`, every second iso-band of width `band` darker, a white zero line of half-width `line`, magenta for NaN.  map
        "count": `values` uint32 (or the int32 tensor `field` returns on the device), the red-green ramp of shade_ranged over
        (lo, hi).  The distance-map defaults are choices for a scene of unit-sized objects, not measured optima.  `rgba`:
        uint8 [..., 4] of values' shape, or None: one is allocated beside `values`.  Returns it.  torch CUDA tensors -> the
        device entry on torch's current stream; numpy arrays -> the host entry (synchronous)."""
        m = N.FIELD_MAPS[map] if isinstance(map, str) else int(map)
        sh = N.rm_field_shade()
        sh.map, sh.reserved = m, 0
        sh.range, sh.band, sh.line = float(range), float(band), float(line)
        sh.lo, sh.hi = int(lo), int(hi)
        on_dev = _is_torch(values)
        if on_dev:
            import torch
            want = (torch.float64,) if m == 0 else (torch.int32, torch.uint32)
            if _bytes_on(True, values) < 0 or values.dtype not in want:
                raise ValueError("values must be a contiguous CUDA tensor of %s" % ("float64" if m == 0 else "int32 / uint32"))
            n = values.numel()
            if rgba is None:
                rgba = torch.empty(tuple(values.shape) + (4,), dtype=torch.uint8, device=values.device)
        else:
            values = np.ascontiguousarray(values, dtype=np.float64 if m == 0 else np.uint32)
            n = values.size
            if rgba is None:
                rgba = np.zeros(values.shape + (4,), np.uint8)
        if _bytes_on(on_dev, rgba) < 4 * n:
            raise ValueError("rgba must be a %s of 4 bytes per value" % ("contiguous CUDA tensor" if on_dev else "writable contiguous numpy array"))
        self._same_device(dict(values=values, rgba=rgba))
        self._both("rm_shade_field", on_dev, C.byref(sh), n, _ptr(values), _ptr(rgba))
        return rgba

    # ---- point queries: distance, normal, object and projection onto the surface ------------
    @staticmethod
    def _point_query(normal, snap, tol, iso, time):
        q = N.rm_point_query()
        q.time, q.iso, q.snap_tol = float(time), float(iso), float(tol)
        q.snap_steps = int(snap)
        q.flags = N.RM_POINT_NORMAL if normal else 0
        return q

    def _points_device(self, q, points, position, want_normal, want_object):
        """rm_scene_points_device on torch's current stream for the CUDA tensor `points` (float32 [n, 3], contiguous); the
        positions go to `position` (which may be `points`).  Returns the other five outputs (None where not asked for)."""
        import torch
        n = points.numel() // 3
        dev = points.device
        dist = torch.empty(n, dtype=torch.float64, device=dev)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_normal else None
        obj = torch.empty(n, dtype=torch.int32, device=dev) if want_object else None
        steps = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)  # (the u32 counts as an int32 tensor, as ray_march's)
        N.check(self._h, N.lib().rm_scene_points_device(self._h, C.byref(q), n, _ptr(points), _ptr(position), _ptr(dist), _ptr(nrm), _ptr(obj),
                                                        _ptr(steps), _ptr(cnt), _current_stream_ptr()))
        return dist, nrm, obj, steps, cnt

    def points(self, points, normal=True, object=True, snap=0, tol=1e-4, iso=0.0, time=0.0, device=False, exact=False):
        """What can be asked about a point (rm_scene_points; the rule is in include/rm_raymarch.h), for float32 [n, 3] points:
        Scene.getDistance there, getNormal's normal, the object that attains the distance, and -- with snap = K > 0 -- the
        point moved onto the surface getDistance == iso by up to K steps of its distance along the normal, until
        |dist - iso| <= tol.  Returns the named tuple Points(position float32 [n, 3], dist float64 [n], normal float32 [n, 3]
        or None, object int32 [n] or None, steps int32 [n], count uint32 [n]), everything taken at `position` (the points as
        given with snap = 0), with the scene at `time`; scene_set_time's value is left alone.  numpy in -> numpy out through
        the host entry (synchronous); a CUDA tensor in, or device=True, -> CUDA tensors through rm_scene_points_device on
        torch's current stream (count an int32 tensor holding the u32 bits).  An empty octree leaf has a constant distance
        and so no gradient, and a BVH's distance over-estimates inside leaf boxes: exact=True (option `exact` for this call)
        answers all of it from the exact field instead, whatever structure the scene has."""
        with self._exact(exact):
            return self._points(points, normal, object, snap, tol, iso, time, device)

    def _points(self, points, normal, object, snap, tol, iso, time, device):
        q = self._point_query(normal, snap, tol, iso, time)
        p = self._device_input("points", points, device, np.float32, (3,), "points must be a contiguous float32 CUDA tensor of [n, 3]")
        if p is not None:
            import torch
            pos = torch.empty((p.numel() // 3, 3), dtype=torch.float32, device=p.device)
            return Points(pos, *self._points_device(q, p, pos, normal, object))
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = len(p)
        pos, dist = np.zeros((n, 3), np.float32), np.zeros(n, np.float64)
        nrm = np.zeros((n, 3), np.float32) if normal else None
        obj = np.zeros(n, np.int32) if object else None
        steps, cnt = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        N.check(self._h, N.lib().rm_scene_points(self._h, C.byref(q), n, _ptr(p), _ptr(pos), _ptr(dist), _ptr(nrm), _ptr(obj), _ptr(steps),
                                                 _ptr(cnt)))
        return Points(pos, dist, nrm, obj, steps, cnt)

    def _device_input(self, name, x, device, dtype, trailing, text):
        """The input of a query that has a device form and a host form: a numpy array without device=True -> None, the host
        entry is to be used; else a contiguous CUDA tensor of `dtype` (a numpy type) and whole rows of `trailing` -- the tensor
        given, which has to be one (ValueError `text`) on the context's device, or the array uploaded as [n] + trailing."""
        if not (_is_torch(x) or device):
            return None
        if self.device < 0:
            raise N.RmError(N.RM_E_NO_DEVICE, "host-only context: there is no CPU distance path")
        if not _is_torch(x):
            import torch
            return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype).reshape((-1,) + trailing)).to(torch.device("cuda", self.device))
        if not (x.is_cuda and str(x.dtype) == "torch." + dtype.__name__ and x.is_contiguous() and x.numel() % (trailing[0] if trailing else 1) == 0):
            raise ValueError(text)
        self._same_device({name: x})
        return x

    def project(self, points, steps=4, tol=1e-4, iso=0.0, time=0.0, device=False, exact=False):
        """The snap alone: `points` moved onto the surface getDistance == iso by up to `steps` steps (points(...) without
        normal and object; exact: as there).  Returns (position, dist, steps)."""
        r = self.points(points, normal=False, object=False, snap=steps, tol=tol, iso=iso, time=time, device=device, exact=exact)
        return r.position, r.dist, r.steps

    def _mesh_attributes(self, vertices, iso, time, snap, tol):
        """The vertices of a mesh (a CUDA tensor) through rm_scene_points_device IN PLACE, K = snap: -> (normals, objects)."""
        if vertices.numel() == 0:
            import torch
            return torch.empty((0, 3), dtype=torch.float32, device=vertices.device), torch.empty(0, dtype=torch.int32, device=vertices.device)
        _, nrm, obj, _, _ = self._points_device(self._point_query(True, snap, tol, iso, time), vertices, vertices, True, True)
        return nrm, obj

    # ---- meshes: the surface of a distance volume, extracted on the device ------------------
    def mesh_field(self, values, origin, du, dv, dw, shape, iso=0.0, device=False, triangles=False, attributes=False, snap=0, tol=1e-4,
                   time=0.0, sharp=False, refine=2, rank_tol=0.1, reach=1.0):
        """Surface nets over a volume the caller already holds (rm_mesh_field_device; the rule is in include/rm_raymarch.h):
        `values` is a torch CUDA tensor or a numpy array of nu * nv * nw float64 or float32 values in the lattice's order
        ([nw, nv, nu]); the surface is where they pass `iso` (inside: value < iso).  The counting call, an exact allocation
        and the filling call, on torch's current stream.  Returns (vertices float32 [V, 3], quads uint32 [Q, 4]): one vertex
        per cell the surface passes through, one quad per lattice edge that changes side, wound so that normals point out of
        the inside -- the winding is flipped here when (du, dv, dw) is left-handed, which the C entry does not do.
        triangles=True returns uint32 [2Q, 3] instead, each quad split (0, 1, 2), (0, 2, 3).  device=True returns torch CUDA
        tensors (the indices an int32 tensor holding the u32 bits).
        attributes=True returns (vertices, faces, normals float32 [V, 3], objects int32 [V]): the vertices have been put
        through rm_scene_points_device in place on the device -- the ACTIVE scene at `time`, this call's iso, K = snap
        projection steps with tolerance tol (0: the vertices as the mesher left them) -- and carry the normal and the object
        there (`points`).  The faces do not depend on it.
        sharp=True moves every vertex to dual contouring's place first (`mesh_cells`, then `sharpen` with refine, rank_tol and
        reach against the ACTIVE scene at `time`): edges and corners of the solid are kept; the faces are untouched and the
        attribute pass runs on the sharpened vertices."""
        lat = self._volume_lattice(origin, du, dv, dw, shape)
        import torch
        values, vt = self._mesh_values(values, lat.nu * lat.nv * lat.nw)

        def call(info, v, n_v, q, n_q):
            N.check(self._h, N.lib().rm_mesh_field_device(self._h, C.byref(lat), _ptr(values), vt, float(iso), v[0], n_v, q[0], n_q, info,
                                                          _current_stream_ptr()))
        (vertices,), (quads,) = self._counted(call, [((3,), torch.float32)], [((4,), torch.int32)])
        cells = self._mesh_cells(lat, values, vt, iso, len(vertices)) if sharp and len(vertices) else None
        return self._finish_mesh(lat, vertices, quads, cells, iso, time, (refine, rank_tol, reach) if sharp else None, triangles, attributes, snap,
                                 tol, device)

    def _need_volume(self, shape):
        if len(tuple(shape)) != 3:
            raise ValueError("a mesh needs a volume: shape is (nu, nv, nw)")
        if self.device < 0:
            raise N.RmError(N.RM_E_NO_DEVICE, "host-only context: there is no CPU mesher")

    def _volume_lattice(self, origin, du, dv, dw, shape, time=0.0):
        """How a mesher opens: a volume's shape, a device, then the rm_lattice."""
        self._need_volume(shape)
        return make_lattice(origin, du, dv, dw, shape, time)

    def _counted(self, call, per_vertex, per_quad=(), counts=None):
        """The capacity protocol of the mesh entries: the counting call, one read of its totals, buffers of exactly the counted
        sizes, the filling call when something was counted.  call(info, vertex_ptrs, n_vertices, quad_ptrs, n_quads) runs the
        entry (a pointer is None in the counting call and for a buffer that is empty or not asked for); per_vertex / per_quad:
        (trailing shape, dtype) per buffer, None for one not asked for.  counts: totals already known, no counting call."""
        import torch
        dev = torch.device("cuda", self.device)
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        if counts is None:
            call(_ptr(info), [None] * len(per_vertex), 0, [None] * len(per_quad), 0)
            counts = info.cpu()[:2].tolist()
        n_v, n_q = counts
        vb = [None if s is None else torch.empty((n_v,) + s[0], dtype=s[1], device=dev) for s in per_vertex]
        qb = [None if s is None else torch.empty((n_q,) + s[0], dtype=s[1], device=dev) for s in per_quad]
        if n_v or n_q:
            call(_ptr(info), [_ptr(b) if n_v else None for b in vb], n_v, [_ptr(b) if n_q else None for b in qb], n_q)
        return vb, qb

    def _finish_mesh(self, lat, vertices, quads, cells, iso, time, sharp, triangles, attributes, snap, tol, device):
        """How a mesh ends, from the device tensors of a mesher: the vertices sharpened (sharp = (refine, rank_tol, reach), with
        the cells' keys) when there are any, the winding flipped when (du, dv, dw) is left-handed, the quads split into
        triangles, the attribute pass on the final vertices, and the download unless `device`."""
        if sharp and len(vertices):
            at = N.rm_lattice.from_buffer_copy(lat)  # (mesh_field's lattice has no time)
            at.time = float(time)
            vertices = self._sharpen_device(at, cells, iso, *sharp, False, False)[0]
        u, v, w = (np.array(list(getattr(lat, k)), np.float64) for k in ("du", "dv", "dw"))
        if float(np.dot(u, np.cross(v, w))) < 0:
            quads = quads[:, [0, 3, 2, 1]].contiguous()
        faces = quads[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3).contiguous() if triangles else quads
        out = (vertices, faces) + (self._mesh_attributes(vertices, iso, time, snap, tol) if attributes else ())
        if device:
            return out
        return (out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32)) + tuple(t.cpu().numpy() for t in out[2:])

    def _mesh_values(self, values, n):
        """`values` as mesh_field takes them -> (a contiguous CUDA tensor of n float64 or float32 values, its RM_MESH_* type)."""
        import torch
        if _is_torch(values):
            if not (values.is_cuda and values.is_contiguous() and values.dtype in (torch.float64, torch.float32)):
                raise ValueError("values must be a contiguous CUDA tensor of float64 or float32")
            self._same_device(dict(values=values))
        else:
            a = np.ascontiguousarray(values)
            values = torch.from_numpy(a if a.dtype == np.float32 else a.astype(np.float64, copy=False)).to(torch.device("cuda", self.device))
        if values.numel() != n:
            raise ValueError("values must hold nu * nv * nw = %d elements" % n)
        return values, (N.RM_MESH_F32 if values.dtype == torch.float32 else N.RM_MESH_F64)

    def _mesh_cells(self, lat, values, vt, iso, n_vertices=None):
        """rm_mesh_cells_device on torch's current stream -> int64 CUDA tensor [V]; n_vertices None: the counting call first."""
        import torch

        def call(info, c, n_v, _, n_q):
            N.check(self._h, N.lib().rm_mesh_cells_device(self._h, C.byref(lat), _ptr(values), vt, float(iso), c[0], n_v, info, _current_stream_ptr()))
        return self._counted(call, [((), torch.int64)], counts=None if n_vertices is None else (n_vertices, 0))[0][0]

    def mesh_cells(self, values, origin, du, dv, dw, shape, iso=0.0, device=False):
        """The cell of every vertex of `mesh_field`'s mesh of the same values (rm_mesh_cells_device): int64 [V], the key
        l = (k * nv + j) * nu + i of the cell's low corner, in vertex order -- what `sharpen` takes, and what the sparse mesher
        returns as `cells`.  device=True returns a CUDA tensor."""
        lat = self._volume_lattice(origin, du, dv, dw, shape)
        values, vt = self._mesh_values(values, lat.nu * lat.nv * lat.nw)
        cells = self._mesh_cells(lat, values, vt, iso)
        return cells if device else cells.cpu().numpy()

    # ---- sharp meshes: vertices from Hermite data ----------------------------------------------
    @staticmethod
    def _sharp_query(iso, refine, rank_tol, reach):
        q = N.rm_sharp_query()
        q.iso, q.rank_tol, q.reach = float(iso), float(rank_tol), float(reach)
        q.refine, q.reserved = int(refine), 0
        return q

    def _sharpen_device(self, lat, cells, iso, refine, rank_tol, reach, want_feature=True, want_count=True):
        """rm_scene_sharpen_device on torch's current stream for the int64 CUDA tensor `cells` -> (position, feature, count)."""
        import torch
        n = cells.numel()
        dev = cells.device
        pos = torch.empty((n, 3), dtype=torch.float32, device=dev)
        feat = torch.empty(n, dtype=torch.int32, device=dev) if want_feature else None
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if want_count else None  # (the u32 counts as an int32 tensor)
        q = self._sharp_query(iso, refine, rank_tol, reach)
        N.check(self._h, N.lib().rm_scene_sharpen_device(self._h, C.byref(lat), C.byref(q), n, _ptr(cells) if n else None, _ptr(pos) if n else None,
                                                         _ptr(feat), _ptr(cnt), _current_stream_ptr()))
        return pos, feat, cnt

    def sharpen(self, cells, origin, du, dv, dw, shape, iso=0.0, time=0.0, refine=2, rank_tol=0.1, reach=1.0, device=False, exact=False):
        """Dual contouring's vertex for the cells `cells` (int64 keys, `mesh_cells`) of a lattice (rm_scene_sharpen; the rule is
        in include/rm_raymarch.h): the point that minimises the distance to the tangent planes of the ACTIVE scene at `time`,
        sampled where the surface getDistance = iso crosses the cell's edges -- each crossing refined `refine` times --, solved
        in the eigenvectors whose eigenvalue exceeds rank_tol times the largest and kept within reach times half a cell's
        diagonal of the cell's centre.  Returns the named tuple Sharp(position float32 [n, 3], feature int32 [n]: 3 a corner, 2
        an edge, 1 a face, 0 the mean of the crossings, -1 no active cell; count uint32 [n]: primitives evaluated).  numpy in
        -> numpy out through the host entry (synchronous); a CUDA tensor in, or device=True, -> CUDA tensors on torch's
        current stream (count an int32 tensor holding the u32 bits).  exact=True: against the exact field, as `points`."""
        if len(tuple(shape)) != 3:
            raise ValueError("a mesh needs a volume: shape is (nu, nv, nw)")
        lat = make_lattice(origin, du, dv, dw, shape, time)
        with self._exact(exact):
            c = self._device_input("cells", cells, device, np.int64, (), "cells must be a contiguous int64 CUDA tensor")
            if c is not None:
                return Sharp(*self._sharpen_device(lat, c, iso, refine, rank_tol, reach))
            c = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1)
            n = len(c)
            pos, feat, cnt = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
            q = self._sharp_query(iso, refine, rank_tol, reach)
            N.check(self._h, N.lib().rm_scene_sharpen(self._h, C.byref(lat), C.byref(q), n, _ptr(c), _ptr(pos), _ptr(feat), _ptr(cnt)))
            return Sharp(pos, feat, cnt)

    def mesh(self, origin, du, dv, dw, shape, iso=0.0, time=0.0, device=False, triangles=False, attributes=False, snap=0, tol=1e-4,
             exact=False, sharp=False, refine=2, rank_tol=0.1, reach=1.0):
        """The surface of the active scene over a lattice: `field` samples Scene.getDistance on the device at `time` (float64,
        once; the volume stays there) and `mesh_field` extracts the surface getDistance = iso from it.  Returns what
        mesh_field returns (attributes, snap, tol: as there).  The field under a BVH or an octree is the marchers' bound, not
        always the exact distance: an offset surface (iso != 0) wants exact=True (option `exact` for this call: the volume
        and the attribute pass then come from the exact field).  sharp, refine, rank_tol, reach: as mesh_field."""
        self._need_volume(shape)  # (field and mesh_field each make the lattice)
        with self._exact(exact):
            vol, _ = self.field(origin, du, dv, dw, shape=shape, time=time, count=False, device=True)
            return self.mesh_field(vol, origin, du, dv, dw, shape, iso=iso, device=device, triangles=triangles, attributes=attributes, snap=snap,
                                   tol=tol, time=time, sharp=sharp, refine=refine, rank_tol=rank_tol, reach=reach)

    # ---- sparse meshes: the same mesh from the 8 x 8 x 8-cell blocks near the surface ---------
    def sparse_blocks(self, origin, du, dv, dw, shape, iso=0.0, time=0.0, lipschitz=1.0, dist=True):
        """The coarse pass of the sparse mesher (rm_scene_blocks_device; the rule is in include/rm_raymarch.h) on torch's
        current stream: one exact distance per block of 8 x 8 x 8 cells, at its centre; a block is kept unless
        |d - iso| > lipschitz * R + slack proves it empty.  Returns the named tuple SparseBlocks(slot int32 [n_blocks]: the
        block's rank among the kept ones or -1, list int32 [n_kept]: the kept blocks in that order, dist float64 [n_blocks] or
        None, n_kept, dims = (nbu, nbv, nbw)); CUDA tensors."""
        import torch
        lat = self._volume_lattice(origin, du, dv, dw, shape, time)
        dims, _, slot, lst = self._block_buffers(lat)
        d = torch.empty(len(slot), dtype=torch.float64, device=slot.device) if dist else None
        n_kept = self._sparse_blocks_into(lat, iso, lipschitz, slot, lst, d)
        return SparseBlocks(slot, lst[:n_kept], d, n_kept, dims)

    def _block_buffers(self, lat):
        """The blocks of a lattice (rm_lattice_blocks) and the two buffers the coarse pass fills -> (dims, n_blocks, slot, list)."""
        import torch
        dims = (C.c_int32 * 3)()
        rc = N.lib().rm_lattice_blocks(C.byref(lat), dims)
        if rc != N.RM_OK:
            raise N.RmError(rc, "rm_lattice_blocks")
        n_blocks = dims[0] * dims[1] * dims[2]
        room = min(n_blocks, 1 << 24)  # (beyond that the entry refuses before it touches a buffer)
        slot = torch.empty(room, dtype=torch.int32, device=torch.device("cuda", self.device))
        return tuple(dims), n_blocks, slot, torch.empty_like(slot)

    def _sparse_blocks_into(self, lat, iso, lipschitz, slot, lst, d=None):
        """The coarse pass into the caller's buffers -> n_kept."""
        import torch
        info = torch.zeros(4, dtype=torch.int64, device=slot.device)
        N.check(self._h, N.lib().rm_scene_blocks_device(self._h, C.byref(lat), float(iso), float(lipschitz), _ptr(slot), _ptr(lst), _ptr(d),
                                                        _ptr(info), _current_stream_ptr()))
        return int(info.cpu()[1])

    def mesh_sparse(self, origin, du, dv, dw, shape, iso=0.0, time=0.0, lipschitz=1.0, order="dense", device=False, triangles=False,
                    attributes=False, snap=0, tol=1e-4, exact=False, sharp=False, refine=2, rank_tol=0.1, reach=1.0):
        """`mesh` from the blocks near the surface only (include/rm_raymarch.h, "sparse meshes"): `sparse_blocks` keeps the
        blocks of 8 x 8 x 8 cells that can hold the surface when the exact field is `lipschitz`-Lipschitz (1 for primitives
        and their unions), rm_scene_tiles_device samples the active scene at the 729 points of each kept block and
        rm_mesh_tiles_device runs surface nets over those tiles (the counting call, an exact allocation, the filling call), all
        on torch's current stream.  Memory and work follow the surface, not the volume: lattices of 512^3 and more points are
        possible.  order="dense" sorts the vertices and the quads by the dense mesher's keys on the device and renames the
        vertices: the result is `mesh`'s, byte for byte, whenever every cell the dense volume has active lies in a kept block
        -- what `lipschitz` guarantees for an exact field.  order="tile" returns the ABI's order, by kept block.  Everything
        else as `mesh` (the winding of a left-handed lattice is flipped here too; exact=True: the tiles and the attribute
        pass come from the exact field, which the coarse pass uses anyway; sharp, refine, rank_tol, reach: as mesh_field, with
        the cell keys the sparse mesher returns itself)."""
        if order not in ("dense", "tile"):
            raise ValueError("order is 'dense' or 'tile'")
        with self._exact(exact):
            return self._mesh_sparse(origin, du, dv, dw, shape, iso, time, lipschitz, order, device, triangles, attributes, snap, tol,
                                     (refine, rank_tol, reach) if sharp else None)

    def _mesh_sparse(self, origin, du, dv, dw, shape, iso, time, lipschitz, order, device, triangles, attributes, snap, tol, sharp=None):
        blocks = self.sparse_blocks(origin, du, dv, dw, shape, iso=iso, time=time, lipschitz=lipschitz, dist=False)
        import torch
        lat = make_lattice(origin, du, dv, dw, shape, time)
        k = blocks.n_kept
        tiles = torch.empty((k, 729), dtype=torch.float64, device=blocks.slot.device)
        self._tiles_into(lat, blocks.list, k, tiles)
        return self._mesh_tiles(lat, blocks.slot, blocks.list, k, tiles, iso, time, order, device, triangles, attributes, snap, tol, sharp)

    def _tiles_into(self, lat, lst, k, tiles):
        """The full tile call (rm_scene_tiles_device): the k kept blocks of `lst` sampled into `tiles`."""
        N.check(self._h, N.lib().rm_scene_tiles_device(self._h, C.byref(lat), _ptr(lst) if k else None, k, _ptr(tiles) if k else None,
                                                       _current_stream_ptr()))

    def _mesh_tiles(self, lat, slot, lst, k, tiles, iso, time, order, device, triangles, attributes, snap, tol, sharp=None):
        """mesh_sparse from the tiles onward (rm_mesh_tiles_device: the counting call, an exact allocation, the filling call):
        slot int32 [n_blocks], lst and tiles hold k kept blocks at least.  What `mesh_sparse` and a MeshSession share."""
        import torch
        dev = torch.device("cuda", self.device)
        dense = order == "dense"

        def call(info, v, n_v, q, n_q):
            N.check(self._h, N.lib().rm_mesh_tiles_device(self._h, C.byref(lat), _ptr(slot), _ptr(lst) if k else None, k, _ptr(tiles) if k else None,
                                                          float(iso), v[0], n_v, q[0], n_q, v[1], q[1], info, _current_stream_ptr()))
        keys = ((), torch.int64)
        (vertices, cells), (quads, edges) = self._counted(call, [((3,), torch.float32), keys if dense or sharp else None],
                                                          [((4,), torch.int32), keys if dense else None])
        n_vertices, n_quads = len(vertices), len(quads)
        if dense and n_vertices:
            by_cell = torch.argsort(cells)  # (the keys are distinct)
            vertices = vertices[by_cell].contiguous()
            cells = cells[by_cell].contiguous()
            rename = torch.empty(n_vertices, dtype=torch.int32, device=dev)
            rename[by_cell] = torch.arange(n_vertices, dtype=torch.int32, device=dev)
            if n_quads:
                quads = rename[quads[torch.argsort(edges)].long()].contiguous()
        return self._finish_mesh(lat, vertices, quads, cells, iso, time, sharp, triangles, attributes, snap, tol, device)

    def mesh_session(self, origin, du, dv, dw, shape, iso=0.0, time=0.0, lipschitz=1.0):
        """A MeshSession over this lattice: the exact sparse mesh of the active scene whose tiles are kept on the device, so
        that after an edit only the tiles the edit can reach are sampled again (include/rm_raymarch.h, "re-meshing an edited
        scene")."""
        return MeshSession(self, origin, du, dv, dw, shape, iso, time, lipschitz)

    def mesh_box(self, cells=(64, 64, 64), margin=None, iso=0.0, time=0.0, device=False, triangles=False, box=None, attributes=False, snap=0,
                 tol=1e-4, sparse=False, lipschitz=1.0, exact=False, sharp=False, refine=2, rank_tol=0.1, reach=1.0):
        """`mesh` over an axis-aligned lattice of cells[0] x cells[1] x cells[2] cells that covers scene_info()'s root box
        and `margin` beyond it on every side (None: two cells and max(iso, 0), so the surface closes inside the lattice).
        `box` = (lo, hi) replaces the root box: a scene without a structure reports none.  sparse=True: `mesh_sparse` with
        `lipschitz` over the same lattice (order "dense": the same mesh).  exact, sharp, refine, rank_tol, reach: as `mesh`."""
        lattice = self._box_lattice(cells, margin, iso, box)
        more = dict(iso=iso, time=time, device=device, triangles=triangles, attributes=attributes, snap=snap, tol=tol, exact=exact, sharp=sharp,
                    refine=refine, rank_tol=rank_tol, reach=reach)
        if sparse:
            more["lipschitz"] = lipschitz
        return (self.mesh_sparse if sparse else self.mesh)(*lattice, **more)

    # ---- measures: how much there is of the solid ---------------------------------------------
    def _read_measure(self, lat, record):
        """The rm_measure a device entry wrote into the int64 CUDA tensor `record` (one read) -> Measure."""
        raw = N.rm_measure.from_buffer_copy(record.cpu().numpy().tobytes())
        return measure_from_record(lat, raw)

    def _measure_values(self, lat, values, vt, iso):
        """rm_measure_field_device on torch's current stream over the CUDA tensor `values` -> Measure."""
        import torch
        record = torch.empty(22, dtype=torch.int64, device=torch.device("cuda", self.device))
        N.check(self._h, N.lib().rm_measure_field_device(self._h, C.byref(lat), _ptr(values) if values.numel() else None, vt, float(iso), _ptr(record),
                                                         _current_stream_ptr()))
        return self._read_measure(lat, record)

    def _measure_tiles(self, lat, slot, lst, k, dist, tiles, iso):
        """rm_measure_tiles_device on torch's current stream over what the coarse pass and a tile pass left -> Measure."""
        import torch
        record = torch.empty(22, dtype=torch.int64, device=torch.device("cuda", self.device))
        N.check(self._h, N.lib().rm_measure_tiles_device(self._h, C.byref(lat), _ptr(slot), _ptr(lst) if k else None, k, _ptr(dist),
                                                         _ptr(tiles) if k else None, float(iso), _ptr(record), _current_stream_ptr()))
        return self._read_measure(lat, record)

    def measure_field(self, values, origin, du, dv, dw, shape, iso=0.0):
        """How much of a volume the caller already holds lies inside (rm_measure_field_device; the rule is in
        include/rm_raymarch.h, "measures"): `values` is a torch CUDA tensor, or a numpy array that is uploaded, of nu * nv * nw
        float64 or float32 values in the lattice's order; a point is inside where value < iso.  shape = (nu, nv) measures a
        slice.  Returns a Measure: the integer fields of rm_measure as Python ints (n_points, n_inside, n_nonfinite, sum1,
        sum2, crossings, lo, hi, n_blocks, n_kept, n_blocks_inside), `.world` (rm_measure_world: cell_volume, volume, centroid,
        second, projected_area, area_estimate) and `.inertia()`.  On torch's current stream; one read of 176 bytes."""
        if self.device < 0:
            raise N.RmError(N.RM_E_NO_DEVICE, "host-only context: there is no CPU measure")
        lat = make_lattice(origin, du, dv, dw, shape)
        values, vt = self._mesh_values(values, lat.nu * lat.nv * lat.nw)
        return self._measure_values(lat, values, vt, iso)

    def measure(self, origin, du, dv, dw, shape, iso=0.0, time=0.0, lipschitz=1.0, sparse=True, exact=True):
        """How much there is of the active scene over a lattice -> Measure (`measure_field`).  sparse=True: `sparse_blocks` with
        its distances, the tiles of the kept blocks under the EXACT field (always: the coarse pass decides by it) and
        rm_measure_tiles_device, on torch's current stream -- work and memory follow the surface; equal to the dense measure
        of the exact field whenever that field is `lipschitz`-Lipschitz.  sparse=False: `field` samples the volume (float64,
        honouring `exact` as `field` does) and `measure_field` measures it."""
        if not sparse:
            vol, _ = self.field(origin, du, dv, dw, shape=shape, time=time, count=False, device=True, exact=exact)
            return self.measure_field(vol, origin, du, dv, dw, shape, iso=iso)
        import torch
        blocks = self.sparse_blocks(origin, du, dv, dw, shape, iso=iso, time=time, lipschitz=lipschitz, dist=True)
        lat = make_lattice(origin, du, dv, dw, shape, time)
        k = blocks.n_kept
        tiles = torch.empty((k, 729), dtype=torch.float64, device=blocks.slot.device)
        with self._exact(True):
            self._tiles_into(lat, blocks.list, k, tiles)
        return self._measure_tiles(lat, blocks.slot, blocks.list, k, blocks.dist, tiles, iso)

    def measure_box(self, cells=(64, 64, 64), margin=None, iso=0.0, time=0.0, box=None, lipschitz=1.0, sparse=True, exact=True):
        """`measure` over `mesh_box`'s lattice: cells[0] x cells[1] x cells[2] cells that cover scene_info()'s root box (or
        `box` = (lo, hi)) and `margin` beyond it on every side."""
        origin, du, dv, dw, shape = self._box_lattice(cells, margin, iso, box)
        return self.measure(origin, du, dv, dw, shape, iso=iso, time=time, lipschitz=lipschitz, sparse=sparse, exact=exact)

    # ---- parts: the connected pieces of the solid, numbered, with a measure each ----------------
    def label_field(self, values, origin, du, dv, dw, shape, iso=0.0, side="inside", records=64, device=False):
        """The connected parts of a volume the caller already holds (rm_label_field_device, then rm_measure_labels_device;
        the rule is in include/rm_raymarch.h, "parts") -> Parts.  `values` as `measure_field` takes them.  side="inside": the
        set is value < iso; "outside": its complement, NaN included; both are 6-connected.  Parts are numbered by their
        smallest linear index.  `records`: how many parts get a Measure (the first ones); None reads n_parts first and sizes
        the records exactly (2^20 at most), a second read.  device=True leaves `.labels` a CUDA tensor.  On torch's current stream; the info
        and the records come back in one read.  A non-zero gave_up raises RmError."""
        if side not in ("inside", "outside"):
            raise ValueError("side is 'inside' or 'outside'")
        if self.device < 0:
            raise N.RmError(N.RM_E_NO_DEVICE, "host-only context: there is no CPU labelling")
        import torch
        lat = make_lattice(origin, du, dv, dw, shape)
        n = lat.nu * lat.nv * lat.nw
        values, vt = self._mesh_values(values, n)
        dev = torch.device("cuda", self.device)
        labels = torch.empty((lat.nw, lat.nv, lat.nu), dtype=torch.int32, device=dev)
        words = C.sizeof(N.rm_measure) // 8
        info = torch.empty(4, dtype=torch.int64, device=dev)

        def measure(k):
            """The info and k records behind it in one int64 tensor, on the host."""
            out = torch.empty(4 + words * k, dtype=torch.int64, device=dev)
            out[:4].copy_(info)
            N.check(self._h, N.lib().rm_measure_labels_device(self._h, C.byref(lat), _ptr(labels) if n else None, k, _ptr(out[4:]) if k else None,
                                                              _current_stream_ptr()))
            return out.cpu().numpy()

        N.check(self._h, N.lib().rm_label_field_device(self._h, C.byref(lat), _ptr(values) if n else None, vt, float(iso),
                                                       N.RM_PARTS_OUTSIDE if side == "outside" else N.RM_PARTS_INSIDE, _ptr(labels) if n else None,
                                                       _ptr(info), _current_stream_ptr()))
        if records is None:
            head = info.cpu().numpy()
            if head[3]:
                raise N.RmError(N.RM_E_HIP, "the labelling gave up: a thread ran out of its hop budget")
            records = min(int(head[2]), 1 << 20)  # what rm_measure_labels_device takes at most
        raw = measure(int(records))
        if raw[3]:
            raise N.RmError(N.RM_E_HIP, "the labelling gave up: a thread ran out of its hop budget")
        n_parts = int(raw[2])
        recs = [N.rm_measure.from_buffer_copy(raw[4 + words * p:4 + words * (p + 1)].tobytes()) for p in range(min(n_parts, int(records)))]
        return Parts(labels if device else labels.cpu().numpy(), int(raw[0]), int(raw[1]), n_parts, [measure_from_record(lat, r) for r in recs], float(iso),
                     side)

    def parts(self, origin, du, dv, dw, shape, iso=0.0, time=0.0, side="inside", records=64, device=False, exact=True):
        """The connected parts of the active scene's solid over a lattice -> Parts (`label_field`): `field` samples the volume
        on the device (float64, honouring `exact` as `field` does) and `label_field` labels and measures it."""
        vol, _ = self.field(origin, du, dv, dw, shape=shape, time=time, count=False, device=True, exact=exact)
        return self.label_field(vol, origin, du, dv, dw, shape, iso=iso, side=side, records=records, device=device)

    def parts_box(self, cells=(64, 64, 64), margin=None, iso=0.0, time=0.0, box=None, side="inside", records=64, device=False, exact=True):
        """`parts` over `mesh_box`'s lattice: cells[0] x cells[1] x cells[2] cells that cover scene_info()'s root box (or
        `box` = (lo, hi)) and `margin` beyond it on every side."""
        origin, du, dv, dw, shape = self._box_lattice(cells, margin, iso, box)
        return self.parts(origin, du, dv, dw, shape, iso=iso, time=time, side=side, records=records, device=device, exact=exact)

    # ---- distances: how far inside the solid every lattice point lies, exactly ------------------
    def edt_field(self, values, origin, du, dv, dw, shape, iso=0.0, side="inside", device=False):
        """The exact Euclidean distance transform of a volume the caller already holds (rm_edt_field_device; the rule is in
        include/rm_raymarch.h, "distances") -> Edt.  `values` as `label_field` takes them.  side="inside": the set is
        value < iso; "outside": its complement, NaN included.  `.d2` is the squared index distance to the nearest lattice
        point on the other side -- points beyond the lattice do not exist, so leave a margin around a solid whose thickness is
        asked.  device=True leaves `.d2` a CUDA tensor.  On torch's current stream; the info comes back in one read."""
        if side not in ("inside", "outside"):
            raise ValueError("side is 'inside' or 'outside'")
        if self.device < 0:
            raise N.RmError(N.RM_E_NO_DEVICE, "host-only context: there is no CPU distance transform")
        import torch
        lat = make_lattice(origin, du, dv, dw, shape)
        n = lat.nu * lat.nv * lat.nw
        values, vt = self._mesh_values(values, n)
        dev = torch.device("cuda", self.device)
        d2 = torch.empty((lat.nw, lat.nv, lat.nu), dtype=torch.int32, device=dev)
        info = torch.empty(4, dtype=torch.int64, device=dev)
        N.check(self._h, N.lib().rm_edt_field_device(self._h, C.byref(lat), _ptr(values) if n else None, vt, float(iso),
                                                     N.RM_PARTS_OUTSIDE if side == "outside" else N.RM_PARTS_INSIDE, _ptr(d2) if n else None, _ptr(info),
                                                     _current_stream_ptr()))
        head = info.cpu().numpy()
        return Edt(d2 if device else d2.cpu().numpy(), head[0], head[1], head[2], head[3], side, lattice_cubic(lat))

    def edt(self, origin, du, dv, dw, shape, iso=0.0, time=0.0, side="inside", device=False, exact=True):
        """The distance transform of the active scene's solid over a lattice -> Edt (`edt_field`): `field` samples the volume
        on the device (float64, honouring `exact` as `field` does) and `edt_field` transforms it."""
        vol, _ = self.field(origin, du, dv, dw, shape=shape, time=time, count=False, device=True, exact=exact)
        return self.edt_field(vol, origin, du, dv, dw, shape, iso=iso, side=side, device=device)

    def edt_box(self, cells=(64, 64, 64), margin=None, iso=0.0, time=0.0, box=None, side="inside", device=False, exact=True):
        """`edt` over `mesh_box`'s lattice: cells[0] x cells[1] x cells[2] cells that cover scene_info()'s root box (or
        `box` = (lo, hi)) and `margin` beyond it on every side -- the margin keeps the solid off the lattice's border, where the
        transform would not see its surface.  The lattice is cubic (`.step`, `.distance()`, `.inradius`) when the cells are."""
        origin, du, dv, dw, shape = self._box_lattice(cells, margin, iso, box)
        return self.edt(origin, du, dv, dw, shape, iso=iso, time=time, side=side, device=device, exact=exact)

    def open_field(self, values, origin, du, dv, dw, shape, r2, iso=0.0, device=False):
        """The morphological opening of the solid value < iso by the squared index radius r2 -> a volume of -1.0 (in the
        result) and +1.0, float64 [nw, nv, nu], a numpy array or a CUDA tensor with device=True.  Two transforms: the set is
        eroded (`Edt.eroded(r2)`: d2 >= r2 stays), then dilated by the same radius -- a point is in the result iff it is in the
        eroded set or its squared distance to the eroded set is below r2.  Crumbs and whiskers thinner than the radius go, the
        rest does not move; the result is always a subset of the solid."""
        import torch
        first = self.edt_field(values, origin, du, dv, dw, shape, iso=iso, side="inside", device=True)
        eroded = first.eroded(r2)
        second = self.edt_field(eroded, origin, du, dv, dw, shape, iso=0.0, side="outside", device=True)
        opened = torch.where((eroded < 0) | (second.d2 < int(r2)), -1.0, 1.0).to(torch.float64)
        return opened if device else opened.cpu().numpy()

    def _box_lattice(self, cells, margin, iso, box):
        """The lattice `mesh_box` meshes over -> (origin, du, dv, dw, shape)."""
        if box is None:
            info = self.scene_info()
            box = (info["root_min"], info["root_max"])
        lo, hi = (np.asarray(b, np.float64).reshape(3) for b in box)
        if not (hi > lo).all():
            raise ValueError("the scene reports no root box (acceleration None): pass box=(lo, hi)")
        c = np.array([int(x) for x in cells], np.int64)
        if (c < 5).any():
            raise ValueError("at least 5 cells per axis")
        m = np.full(3, float(margin)) if margin is not None else max(float(iso), 0.0) * (1 + 4 / (c - 4)) + 2 * (hi - lo) / (c - 4)
        step = (hi - lo + 2 * m) / c
        return lo - m, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), tuple(int(x) + 1 for x in c)

    def _same_device(self, bufs):
        for name, b in bufs.items():
            if b is not None and _is_torch(b) and b.is_cuda and b.device.index != self.device:
                raise ValueError("%s buffer is on cuda:%s, the context on cuda:%d" % (name, b.device.index, self.device))

    def _both(self, name, on_dev, *args):
        """The two forms of an entry from one argument list: <name>_device on torch's current stream for device buffers, <name>
        (synchronous) for host buffers."""
        if on_dev:
            N.check(self._h, getattr(N.lib(), name + "_device")(self._h, *args, _current_stream_ptr()))
        else:
            N.check(self._h, getattr(N.lib(), name)(self._h, *args))

    def render_stripes(self, job, stripe_rows, n_parts, part, depth, normal, sdf, iters, rgba=None, shader=0, diag=None):
        """One launch for every stripe of `part` (rm_render_stripes_device); device buffers only."""
        rows = N.lib().rm_stripe_rows(job.y_start, job.y_end, int(stripe_rows), int(n_parts), int(part))
        if rows < 0:
            raise ValueError("bad stripe partition")
        bufs = dict(depth=depth, normal=normal, sdf=sdf, iters=iters, rgba=rgba)
        _check_buffers(rows * max(0, job.width), bufs, need_device=True)
        self._same_device(bufs)
        self._attach_diag(diag)
        N.check(self._h, N.lib().rm_render_stripes_device(
            self._h, C.byref(job), int(shader), int(stripe_rows), int(n_parts), int(part), _ptr(depth), _ptr(normal),
            _ptr(sdf), _ptr(iters), _ptr(rgba), _current_stream_ptr()))

    def render_stripe_list(self, job, stripe_rows, stripe_ids, depth, normal, sdf, iters, rgba=None, shader=0, diag=None):
        """One launch for the listed stripes (strictly increasing ids; rm_render_stripe_list_device), packed in list
        order; device buffers only.  Serves any deal of stripes to ranks (deal_stripes)."""
        ids = np.ascontiguousarray(stripe_ids, dtype=np.int32)
        height = max(0, job.y_end - job.y_start)
        rows = sum(min(height, (int(i) + 1) * stripe_rows) - int(i) * stripe_rows for i in ids)
        bufs = dict(depth=depth, normal=normal, sdf=sdf, iters=iters, rgba=rgba)
        _check_buffers(max(0, rows) * max(0, job.width), bufs, need_device=True)
        self._same_device(bufs)
        self._attach_diag(diag)
        N.check(self._h, N.lib().rm_render_stripe_list_device(
            self._h, C.byref(job), int(shader), int(stripe_rows), _ptr(ids), len(ids), _ptr(depth), _ptr(normal),
            _ptr(sdf), _ptr(iters), _ptr(rgba), _current_stream_ptr()))

    def assemble_frame(self, gathered, rank_stride, section_offset, row_bytes, height, stripe_rows, owner, world, frame,
                       acc_offset=-1, acc=None):
        """Rank 0's fan-in in one kernel (rm_assemble_frame_device): stripes of the gathered per-rank buffers -> row-major
        frame, and the ranks' 32-byte partial diagnostics (at acc_offset of each rank's buffer) -> acc."""
        own = np.ascontiguousarray(owner, dtype=np.int32)
        for name, t, need in (("gathered", gathered, world * rank_stride), ("frame", frame, row_bytes * height)):
            if not (_is_torch(t) and t.is_cuda and t.is_contiguous()) or t.numel() * t.element_size() < need:
                raise ValueError("%s must be a contiguous CUDA tensor of at least %d bytes" % (name, need))
        if acc is not None and (not (_is_torch(acc) and acc.is_cuda) or acc.numel() * acc.element_size() < 32):
            raise ValueError("acc must be a CUDA tensor of 32 bytes")
        N.check(self._h, N.lib().rm_assemble_frame_device(
            self._h, _ptr(gathered), int(rank_stride), int(section_offset), int(row_bytes), int(height), int(stripe_rows),
            _ptr(own), len(own), int(world), _ptr(frame), int(acc_offset), _ptr(acc), _current_stream_ptr()))

    def last_kernel(self):
        """The render-kernel instantiation the last render entry launched (rm_last_kernel)."""
        return N.lib().rm_last_kernel(self._h).decode()

    # ---- run-time specialised kernels of expression forests (rm_rtc_*) -------------------
    def rtc_source(self):
        """The straight-line HIP source generated for the active scene's expression forest ("" if none)."""
        need = C.c_int64(0)
        N.check(self._h, N.lib().rm_rtc_source(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(max(1, need.value))
        N.check(self._h, N.lib().rm_rtc_source(self._h, buf, len(buf), None))
        return buf.value.decode()

    def rtc_compile_check(self, accel=0, other=False, refused_ok=False):
        """Compiles the active scene's specialised kernel for gfx950 without loading it (no GPU needed).
        Returns (compiler log with the resource-usage remarks, seconds).  A kernel that spills a VGPR is refused, as a
        render would refuse it (the interpreter kernel then serves the scene): RuntimeError, or with refused_ok the
        log -- it then starts with "refused:"."""
        buf = C.create_string_buffer(1 << 16)
        secs = C.c_double(0)
        rc = N.lib().rm_rtc_compile_check(self._h, int(accel), int(bool(other)), buf, len(buf), C.byref(secs))
        if rc == N.RM_E_UNSUPPORTED and refused_ok and buf.value.startswith(b"refused:"):
            return buf.value.decode(), secs.value
        if rc != 0:
            raise RuntimeError("rm_rtc_compile_check: %s\n%s" % (N.lib().rm_last_error(self._h).decode(), buf.value.decode()))
        return buf.value.decode(), secs.value

    def rtc_status(self):
        """(kernels compiled for the active scene, compiles that failed, most recent compile log)."""
        done, bad = C.c_int32(0), C.c_int32(0)
        buf = C.create_string_buffer(1 << 16)
        N.check(self._h, N.lib().rm_rtc_status(self._h, C.byref(done), C.byref(bad), buf, len(buf)))
        return done.value, bad.value, buf.value.decode()

    def shade(self, shader, width, height, depth, normal, sdf, iters, rgba):
        npx = max(0, int(width)) * max(0, int(height))
        bufs = dict(depth=depth, normal=normal, sdf=sdf, iters=iters, rgba=rgba)
        if depth is None or normal is None or sdf is None or iters is None or rgba is None:
            raise ValueError("shade needs all five buffers")
        on_dev = _check_buffers(npx, bufs)
        if on_dev:
            self._same_device(bufs)
        self._both("rm_shade", on_dev, int(shader), width, height, _ptr(depth), _ptr(normal), _ptr(sdf), _ptr(iters), _ptr(rgba))

    def _check_counters(self, sdf, iters):
        if sdf is None or iters is None:
            raise ValueError("null counter buffer")
        n = int(sdf.numel()) if _is_torch(sdf) else int(sdf.size)
        m = int(iters.numel()) if _is_torch(iters) else int(iters.size)
        if n != m:
            raise ValueError("sdfEval and iters differ in length (%d, %d)" % (n, m))
        dev = _check_buffers(n, dict(sdf=sdf, iters=iters))
        if dev:
            self._same_device(dict(sdf=sdf, iters=iters))
        return n, dev

    def reduce_counters(self, sdf, iters):
        out = N.rm_diagnostics()
        n, dev = self._check_counters(sdf, iters)
        if dev:
            N.check(self._h, N.lib().rm_reduce_counters_device(self._h, _ptr(sdf), _ptr(iters), n,
                                                                C.byref(out), _current_stream_ptr()))
        else:
            N.check(self._h, N.lib().rm_reduce_counters(self._h, _ptr(sdf), _ptr(iters), n, C.byref(out)))
        return {"total_sdf": int(out.total_sdf_calls), "total_iters": int(out.total_iterations),
                "max_sdf": int(out.max_sdf_calls), "min_sdf": int(out.min_sdf_calls),
                "total_pixels": int(out.total_pixels)}

    def reduce_counters_enqueue(self, sdf, iters, acc):
        """Async diagnostics for a frame loop: `acc` is a CUDA int64[4] tensor that receives
        (total_sdf, total_iters, max_sdf | min_sdf << 32, pad); read it with decode_acc()."""
        n, dev = self._check_counters(sdf, iters)
        if not dev and n:
            raise ValueError("reduce_counters_enqueue takes device buffers")
        if not (_is_torch(acc) and acc.is_cuda and acc.numel() * acc.element_size() >= 32):
            raise ValueError("acc must be a CUDA tensor of 32 bytes")
        N.check(self._h, N.lib().rm_reduce_counters_enqueue(self._h, _ptr(sdf), _ptr(iters), n,
                                                            _ptr(acc), _current_stream_ptr()))

    @staticmethod
    def decode_acc(acc):
        v = [int(x) for x in acc.cpu().tolist()]
        return {"total_sdf": v[0], "total_iters": v[1], "max_sdf": v[2] & 0xFFFFFFFF,
                "min_sdf": (v[2] >> 32) & 0xFFFFFFFF}

    @staticmethod
    def decode_accs(acc):
        """decode_acc for a batch: one dict per 32-byte accumulator of `acc` (render_frames' diag)."""
        v = acc.cpu().contiguous().view(-1).numpy().view(np.uint64).reshape(-1, 4)
        return [{"total_sdf": int(r[0]), "total_iters": int(r[1]), "max_sdf": int(r[2]) & 0xFFFFFFFF, "min_sdf": int(r[2]) >> 32}
                for r in v]

    def selftest_hypot(self, xyz):
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(a), np.float64)
        N.check(self._h, N.lib().rm_selftest_hypot(self._h, _ptr(a), len(a), _ptr(out)))
        return out


def _selftest_fastdiv(self, seed, n):
    """Device-side comparison of the two Math.hypot forms; returns the mismatch count."""
    out = C.c_uint64(0)
    N.check(self._h, N.lib().rm_selftest_fastdiv(self._h, int(seed), int(n), C.byref(out)))
    return out.value


Context.selftest_fastdiv = _selftest_fastdiv


def _selftest_recip(self, mode):
    """Exhaustive device-side check of the range-restricted division of ray set-up (mode 0: 1.0 / d for every finite
    non-zero binary32 d; mode 1: x / W for 0 <= x < 65536, 1 <= W < 65536); returns the mismatch count."""
    out = C.c_uint64(0)
    N.check(self._h, N.lib().rm_selftest_recip(self._h, int(mode), C.byref(out)))
    return out.value


Context.selftest_recip = _selftest_recip


def make_lattice(origin, du, dv, dw=None, shape=(1, 1), time=0.0):
    """An rm_lattice: point (i, j, k) = origin + i * du + j * dv + k * dw (float32 vectors; dw None: zero), shape (nu, nv) or
    (nu, nv, nw), the query's time."""
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (2, 3):
        raise ValueError("shape is (nu, nv) or (nu, nv, nw)")
    lat = N.rm_lattice()
    for name, v in (("origin", origin), ("du", du), ("dv", dv), ("dw", (0, 0, 0) if dw is None else dw)):
        getattr(lat, name)[:] = [float(x) for x in np.asarray(v, np.float32).reshape(3)]
    lat.nu, lat.nv, lat.nw = shape[0], shape[1], (shape[2] if len(shape) == 3 else 1)
    if min(lat.nu, lat.nv, lat.nw) < 0 or max(lat.nu, lat.nv, lat.nw) > 65535:
        raise ValueError("lattice counts must be in [0, 65535]")
    lat.reserved = 0
    lat.time = float(time)
    return lat


def measure_world(lat, record):
    """rm_measure_world (host-only, no context): the N.rm_measure `record` in the world units of the rm_lattice `lat` ->
    MeasureWorld(cell_volume, volume, centroid[3], second[6] as xx yy zz xy yz zx, projected_area[3], area_estimate)."""
    out = N.rm_measure_world()
    rc = N.lib().rm_measure_world(C.byref(lat), C.byref(record), C.byref(out))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_measure_world")
    return MeasureWorld(out.cell_volume, out.volume, tuple(out.centroid), tuple(out.second), tuple(out.projected_area), out.area_estimate)


def lattice_cubic(lat):
    """rm_lattice_cubic of an rm_lattice: the length of its steps where they are equal and orthogonal to 1e-5 (axes of one
    point aside), so that index distances are world distances up to this factor; else None."""
    step = C.c_double(0.0)
    rc = N.lib().rm_lattice_cubic(C.byref(lat), C.byref(step))
    if rc == N.RM_E_UNSUPPORTED:
        return None
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_lattice_cubic refused the lattice")
    return step.value


def measure_from_record(lat, record):
    """An N.rm_measure over the rm_lattice `lat` -> Measure, its `world` filled in."""
    m = Measure(record.n_points, record.n_inside, record.n_nonfinite, tuple(record.sum1), tuple(record.sum2), tuple(record.crossings),
                tuple(record.lo), tuple(record.hi), record.n_blocks, record.n_kept, record.n_blocks_inside)
    m.world = measure_world(lat, record)
    return m


def slice_lattice(axis="z", offset=0.0, half_extent=5.0, size=(256, 256)):
    """The lattice of the axis-aligned plane axis = offset, [-half_extent, half_extent] in both other axes, sampled at the
    centres of size = (nu, nv) texels -> (origin, du, dv, (nu, nv)), float32 vectors, what Context.field takes.  i runs along
    x (y for axis "x"), j along y (z for axes "x" and "y")."""
    a = {"x": 0, "y": 1, "z": 2}[axis]
    u, v = [c for c in range(3) if c != a]
    nu, nv = int(size[0]), int(size[1])
    h = float(half_extent)
    su, sv = 2.0 * h / max(nu, 1), 2.0 * h / max(nv, 1)
    origin, du, dv = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    origin[a], origin[u], origin[v] = offset, -h + 0.5 * su, -h + 0.5 * sv
    du[u], dv[v] = su, sv
    return origin, du, dv, (nu, nv)


def make_transform(x, y, z, rotation=None):
    """SceneManager.getTransform (sceneManager.ts:21-37) -> world->local float32[16]."""
    out = np.zeros(16, np.float32)
    rot = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float32)
    rc = N.lib().rm_make_transform(float(x), float(y), float(z), _ptr(rot), _ptr(out))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_make_transform")
    return out


def scale_transform(m, x, y, z):
    """gl-matrix mat4.scale(m, m, [x, y, z]) (sceneManager.ts:63) -> new float32[16]."""
    out = np.ascontiguousarray(m, dtype=np.float32).copy()
    rc = N.lib().rm_scale_transform(_ptr(out), float(x), float(y), float(z))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_scale_transform")
    return out


def camera_from_angles(pitch, yaw):
    rot = np.zeros(9, np.float32)
    org = np.zeros(3, np.float32)
    rc = N.lib().rm_camera_from_angles(float(pitch), float(yaw), _ptr(rot), _ptr(org))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_camera_from_angles")
    return rot, org


def sweep_views(pitch, yaw, d_pitch, d_yaw, time0=0.0, d_time=0.0, n=1):
    """rm_sweep_views: the (pitch, yaw, time) of Camera.setAngles(pitch, yaw) followed by n - 1 calls of
    Camera.rotateCamera(d_pitch, d_yaw) (camera.ts:26-31,58-62), time0 + k * d_time -> float64 (n, 3), what
    Context.render_frames takes as views."""
    out = np.zeros((max(0, int(n)), 3), np.float64)
    rc = N.lib().rm_sweep_views(float(pitch), float(yaw), float(d_pitch), float(d_yaw), float(time0), float(d_time), int(n), _ptr(out))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_sweep_views")
    return out


def camera_rays(width, height, pitch, yaw, y_start=0, y_end=None):
    """rm_camera_rays: the rays runRaymarcher casts for rows [y_start, y_end) of a width x height frame
    (raymarcher.ts:61-88) -> (origin float32[3], directions float32[(y_end - y_start) * width, 3])."""
    if y_end is None:
        y_end = height
    org = np.zeros(3, np.float32)
    dirs = np.zeros((max(0, int(y_end) - int(y_start)) * max(0, int(width)), 3), np.float32)
    rc = N.lib().rm_camera_rays(int(width), int(height), float(pitch), float(yaw), int(y_start), int(y_end), _ptr(org), _ptr(dirs))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_camera_rays")
    return org, dirs


def phong_light():
    """rm_phong_light: the binary32 light direction PhongModel normalises from (1, -1, 1.5) (phongModel.ts:15-16) ->
    float32[3]; what the "phong" shader and Context.shade_lit shade with, and Context.light's default direction."""
    out = np.zeros(3, np.float32)
    rc = N.lib().rm_phong_light(_ptr(out))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_phong_light")
    return out


def deal_stripes(rows, stripe_rows, n_parts, weights=None):
    """rm_deal_stripes: owner of every stripe of `rows` rows (smooth weighted round-robin; equal weights = round-robin)."""
    n = (max(0, int(rows)) + int(stripe_rows) - 1) // int(stripe_rows)
    owner = np.zeros(max(1, n), np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
    if w is not None and len(w) != n_parts:
        raise ValueError("one weight per part")
    rc = N.lib().rm_deal_stripes(int(rows), int(stripe_rows), int(n_parts), _ptr(w), _ptr(owner))
    if rc < 0:
        raise N.RmError(rc, "rm_deal_stripes")
    return owner[:rc]


def partition_rows(height, n_workers, i):
    """main.ts:444-449."""
    a, b = C.c_int32(0), C.c_int32(0)
    rc = N.lib().rm_partition_rows(int(height), int(n_workers), int(i), C.byref(a), C.byref(b))
    if rc != N.RM_OK:
        raise N.RmError(rc, "rm_partition_rows")
    return a.value, b.value


class MeshSession:
    """The exact sparse mesh of a context's active scene over one lattice, kept up to date across edits (Context.mesh_session;
    the rule is in include/rm_raymarch.h, "re-meshing an edited scene").  It owns two sets of (slot, list, tiles) on the
    device: the current one, which `mesh` reads, and the one the next update writes while it copies from the current one.
    Everything runs on torch's current stream.  `stats`: the last update's rm_tiles_update_info as a dict (n_kept, n_reused,
    n_evaluated)."""

    def __init__(self, ctx, origin, du, dv, dw, shape, iso=0.0, time=0.0, lipschitz=1.0):
        self.lattice = ctx._volume_lattice(origin, du, dv, dw, shape, time)
        import torch
        self.ctx, self.iso, self.time, self.lipschitz = ctx, float(iso), float(time), float(lipschitz)
        dev = torch.device("cuda", ctx.device)
        # [slot, list, tiles, n_kept, dist] twice; the tiles grow with the kept set
        self._sets = []
        for _ in range(2):
            self.dims, self.n_blocks, slot, lst = ctx._block_buffers(self.lattice)
            self._sets.append([slot, lst, torch.empty((0, 729), dtype=torch.float64, device=dev), 0, torch.empty(len(slot), dtype=torch.float64, device=dev)])
        self._cur = None  # index of the current set
        self._info = torch.zeros(4, dtype=torch.int64, device=dev)
        self.reused = None  # int32 [n_kept]: the last update's flags (1: the tile was copied), on the device
        self.stats = None
        self.update(None)

    @property
    def slot(self):
        return self._sets[self._cur][0]

    @property
    def list(self):
        s = self._sets[self._cur]
        return s[1][:s[3]]

    @property
    def tiles(self):
        s = self._sets[self._cur]
        return s[2][:s[3]]

    @property
    def n_kept(self):
        return self._sets[self._cur][3]

    def update(self, balls=None):
        """Brings the tiles up to the ACTIVE scene: a fresh coarse pass, then rm_scene_tiles_update_device with `balls` -- a
        record array of N.BALL_DTYPE (Context.edit_balls), or a sequence of (centre[3], radius) -- that cover every object
        version the scenes differ by; then the sets swap.  balls=None: every kept block is sampled again (the full exact
        path: what a caller who changed the scene in ways no ball describes asks for, and what a forest always takes)."""
        import torch
        ctx, lat = self.ctx, self.lattice
        target = 1 - self._cur if self._cur is not None else 0
        new = self._sets[target]
        k = ctx._sparse_blocks_into(lat, self.iso, self.lipschitz, new[0], new[1], new[4])
        if new[2].shape[0] < k:
            new[2] = torch.empty((k + k // 8, 729), dtype=torch.float64, device=new[0].device)
        new[3] = k
        if balls is None or self._cur is None:
            with ctx._exact(True):
                ctx._tiles_into(lat, new[1], k, new[2])
            self.reused = torch.zeros(k, dtype=torch.int32, device=new[0].device)
            self.stats = dict(n_kept=k, n_reused=0, n_evaluated=k)
        else:
            if not (isinstance(balls, np.ndarray) and balls.dtype == np.dtype(N.BALL_DTYPE)):
                rec = np.zeros(len(balls), N.BALL_DTYPE)
                for i, (centre, radius) in enumerate(balls):
                    rec[i]["center"], rec[i]["radius"] = np.asarray(centre, np.float32).reshape(3), float(radius)
                balls = rec
            n = len(balls)
            d_balls = torch.from_numpy(np.ascontiguousarray(balls).view(np.uint8).reshape(-1).copy()).to(new[0].device) if n else None
            old = self._sets[self._cur]
            self.reused = torch.empty(k, dtype=torch.int32, device=new[0].device)
            N.check(ctx._h, N.lib().rm_scene_tiles_update_device(
                ctx._h, C.byref(lat), _ptr(old[0]), _ptr(old[2]) if old[3] else None, old[3], _ptr(d_balls), n, _ptr(new[1]) if k else None, k,
                _ptr(new[2]) if k else None, _ptr(self.reused) if k else None, _ptr(self._info), _current_stream_ptr()))
            info = [int(x) for x in self._info.cpu()]
            self.stats = dict(n_kept=info[0], n_reused=info[1], n_evaluated=info[2])
        self._cur = target
        return self.stats

    def edit_spheres(self, edits):
        """Context.edit_spheres, then the update with the edits' own balls (Context.edit_balls).  All or nothing as the edit is:
        a refused edit leaves the scene and the session as they were."""
        edits = edits if isinstance(edits, C.Array) else list(edits)
        balls = self.ctx.edit_balls(edits)
        self.ctx.edit_spheres(edits)
        return self.update(balls)

    def mesh(self, order="dense", triangles=False, device=False):
        """The mesh of the current tiles: what Context.mesh_sparse(exact=True) returns for the active scene over the session's
        lattice, byte for byte, without its coarse pass and its tile pass."""
        if order not in ("dense", "tile"):
            raise ValueError("order is 'dense' or 'tile'")
        s = self._sets[self._cur]
        return self.ctx._mesh_tiles(self.lattice, s[0], s[1], s[3], s[2], self.iso, self.time, order, device, triangles, False, 0, 1e-4)

    def measure(self):
        """The Measure of the current tiles (rm_measure_tiles_device): what Context.measure(sparse=True) returns for the active
        scene over the session's lattice, without its coarse pass and its tile pass."""
        s = self._sets[self._cur]
        return self.ctx._measure_tiles(self.lattice, s[0], s[1], s[3], s[4], s[2], self.iso)
