"""The host form of a ray query past one chunk of its scratch staging (rm_api.cpp, ray_call): a batch of 2^22 + 257 rays takes
the chunk loop round twice, with a short second trip.  Every output of the host entry equals the device entry's on the same
rays byte for byte, and the rays either side of the chunk boundary equal themselves as single-ray host calls.  Pick (whose
columns are a superset of the march's) and light; light once more with two outputs absent, whose columns then take no region
of the scratch.  A one-primitive scene without acceleration: the march is a few iterations per ray, the test is copies."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHUNK = 1 << 22
N_RAYS = CHUNK + 257
SLICE = 200003  # rays per call of the device entry: the host form's scratch is the only large device buffer (under 300 MB with it)
FILL = 0xA5
COLUMNS = {
    "pick": (("t", np.float64, 1), ("iters", np.uint32, 1), ("sdf_calls", np.uint32, 1), ("normal", np.float32, 3), ("object", np.int32, 1)),
    "light": (("t", np.float64, 1), ("iters", np.uint32, 1), ("sdf_calls", np.uint32, 1), ("normal", np.float32, 3), ("lit", np.float32, 1),
              ("ao", np.float32, 1), ("iters2", np.uint32, 1), ("sdf_calls2", np.uint32, 1)),
}


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def cctx(rm):
    ctx = rm.Context(0)
    rm.Scene("None", ctx=ctx).loadPreset(0)
    return ctx


@pytest.fixture(scope="module")
def rays():
    from test_ray_queries import random_rays
    o, d = random_rays(N_RAYS, seed=22)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def host_entry(rm, ctx, family, o, d, out):
    """rm_ray_pick / rm_ray_light with Context.pick's / Context.light's defaults; out: one array or None per column."""
    N = rm._native
    q = N.rm_ray_query()
    q.algorithm = N.lib().rm_algorithm_from_string(b"sphere-tracer")
    q.normal = 1
    q.time = 0.0
    q.overshoot_factor = q.step_size = float("nan")
    if family == "pick":
        rc = N.lib().rm_ray_pick(ctx._h, C.byref(q), len(o), vp(o), vp(d), *[vp(b) for b in out])
    else:
        lt = N.rm_light()
        lt.dir[:] = [float(v) for v in rm.phong_light()]
        lt.ao_samples, lt.bias, lt.ao_step, lt.ao_strength = 5, 0.02, 0.05, 1.0
        rc = N.lib().rm_ray_light(ctx._h, C.byref(q), C.byref(lt), len(o), vp(o), vp(d), *[vp(b) for b in out])
    N.check(ctx._h, rc)


def device_entry(ctx, family, o, d):
    """Context.pick / Context.light on CUDA tensors of the rays -> the columns as numpy arrays."""
    import torch
    got = getattr(ctx, family)(torch.tensor(o).cuda(), torch.tensor(d).cuda())  # (copies: the rays are read-only arrays)
    return [g.cpu().numpy() for g in got]


@pytest.mark.gpu
@pytest.mark.parametrize("family,absent", [("pick", ()), ("light", ()), ("light", ("t", "iters2"))])
def test_a_host_batch_crosses_the_chunk_of_the_host_form(rm, cctx, rays, family, absent):
    o, d = rays
    cols = COLUMNS[family]
    bufs = [np.full(N_RAYS * w * np.dtype(dt).itemsize, FILL, np.uint8).view(dt).reshape(N_RAYS, w) for _, dt, w in cols]
    host_entry(rm, cctx, family, o, d, [None if name in absent else b for (name, _, _), b in zip(cols, bufs)])
    for (name, _, _), b in zip(cols, bufs):  # a column that was not asked for: its buffer was never given, and nothing reached it
        if name in absent:
            assert (b.view(np.uint8) == FILL).all(), name
    for s in range(0, N_RAYS, SLICE):
        for (name, _, _), b, g in zip(cols, bufs, device_entry(cctx, family, o[s:s + SLICE], d[s:s + SLICE])):
            if name not in absent:
                assert b[s:s + SLICE].tobytes() == g.tobytes(), (name, s)
    for i in (0, CHUNK - 1, CHUNK, N_RAYS - 1):
        one = [np.zeros((1, w), dt) for _, dt, w in cols]
        host_entry(rm, cctx, family, o[i:i + 1], d[i:i + 1], [None if name in absent else b for (name, _, _), b in zip(cols, one)])
        for (name, _, _), b, x in zip(cols, bufs, one):
            if name not in absent:
                assert b[i:i + 1].tobytes() == x.tobytes(), (name, i)
