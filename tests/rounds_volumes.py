"""The lattices and volumes of tests/test_lattice_rounds.py and tests/test_lattice_rounds_gpu.py: shapes at which the loops of
rm_measure.hip, rm_parts.hip and rm_edt.hip take a second and later iteration, the volumes that reach their branches, and the
counts that say so -- from the header's constants and the lattice alone, never from the code under test."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 266 265 and 273 504 points: 1 041 and 1 069 workgroups of 256, 4 161 and 4 274 chunks of 64; a row of the second is four
# waves and three points
BIG = [(97, 61, 45), (259, 33, 32)]
# 8 777 rows; a chunk loop of three iterations; nv = 2
ROWS = [(5, 131, 67), (300, 9, 5), (3, 2, 20000)]
# the largest index on each axis
LONG = [(65535, 2, 1), (1, 65535, 2), (2, 1, 65535)]
# preset 0 (a sphere of radius 1.5 about the origin) over x, y in [-0.2, 0.2], z in [-1, 2]: blocks 1 x 1 x 8 191
SPARSE = ((-0.2, -0.2, -1.0), (0.4 / 8, 0, 0), (0, 0.4 / 8, 0), (0, 0, 3.0 / 65528), (9, 9, 65529))

WAVE = 64
FIELD_CHUNK = 128  # measure_field_kernel takes two chunks of 64 points of a row a step


def constants():
    """RM_MESH_BLOCK, RM_MESH_SCAN_STEP and the workgroups edt_reduce_kernel has at most (RM_EDT_PARTIAL_BYTES / 16)."""
    text = open(os.path.join(ROOT, "cpu_raymarcher_amd", "csrc", "rm_kernels.h")).read()
    block, step = (int(re.search(r"#define %s (\d+)" % k, text).group(1)) for k in ("RM_MESH_BLOCK", "RM_MESH_SCAN_STEP"))
    each, most = (int(x) for x in re.search(r"#define RM_EDT_PARTIAL_BYTES \((\d+) \* (\d+)\)", text).groups())
    assert each == 16  # two 64-bit words a partial
    return block, step, most


def ceil_div(a, b):
    return -(-a // b)


def size(shape):
    return shape[0] * shape[1] * shape[2]


# ------------------------------------------------------------------------------------------------- volumes

def random_measure_values(shape, dtype, seed=7):
    """The measure tests' recipe at (67, 10, 21): normal values about iso = 0.25, a fifth equal to iso, NaN and both infinities."""
    v = np.random.default_rng(seed + shape[0]).standard_normal(size(shape))
    v[::5] = 0.25
    v[3], v[11], v[20] = float("nan"), float("inf"), float("-inf")
    return v.astype(dtype)


def random_set_values(shape, density, dtype, seed=0):
    """The parts tests' recipe: values about iso = 0.25 of which `density` lie below; some equal iso, one NaN, both infinities."""
    v = np.random.default_rng(seed + shape[0] + 7 * shape[1]).random(size(shape)) - density + 0.25
    v[::7] = 0.25
    v[3], v[5], v[9] = float("nan"), float("inf"), float("-inf")
    return v.astype(dtype)


def unit_coordinates(shape):
    """x, y, z in [0, 1] over the lattice, broadcastable to [nw, nv, nu]; None for an axis of fewer than 8 points."""
    nu, nv, nw = shape
    axis = lambda n: np.arange(n, dtype=np.float64) / (n - 1) if n >= 8 else None  # noqa: E731
    x, y, z = axis(nu), axis(nv), axis(nw)
    return (None if x is None else x.reshape(1, 1, nu), None if y is None else y.reshape(1, nv, 1), None if z is None else z.reshape(nw, 1, 1))


def two_balls(shape):
    """A smooth volume, negative inside: two balls of the unit cube the lattice spans (ellipsoids in index units) of radius 0.22
    about (0.3, 0.35, 0.3) and (0.7, 0.6, 0.7).  They do not touch: their centres are 0.62 apart.  An axis of fewer than 8
    points does not count: the balls are cylinders along it."""
    def ball(centre):
        terms = [(c - at) ** 2 for c, at in zip(unit_coordinates(shape), centre) if c is not None]
        return np.sqrt(sum(terms)) - 0.22
    return np.minimum(ball((0.3, 0.35, 0.3)), ball((0.7, 0.6, 0.7))) + np.zeros((shape[2], shape[1], shape[0]))


def few_pieces(shape):
    """The two balls and a third piece of 2 x 2 x 3 points far along k, behind the second ball (which ends at 0.92 of the axis)."""
    v = two_balls(shape)
    nw = shape[2]
    assert (v[nw - 3:] > 0).all()
    v[nw - 3:nw - 1, 2:4, 2:5] = -1.0
    return v


def two_slabs(shape):
    """Two parts that follow one another closely in linear order: the rows j < nv / 2 of every plane and the rows j > nv / 2,
    a wall row between them.  The last row of a plane belongs to the second, the first row of the next plane to the first; 20
    points at either side of that seam lie outside, so a seam is a gap of 40 points between two labels.  Where a multiple of 64
    falls into the gap, the chunk ahead holds the second label alone and the chunk behind the first alone."""
    nu, nv, nw = shape
    assert nu > 40 and nv >= 5
    v = np.full((nw, nv, nu), -1.0)
    v[:, nv // 2, :] = 1.0
    v[:, 0, :20] = 1.0
    v[:, nv - 1, nu - 20:] = 1.0
    return v


def disc_at_the_end(shape, radius):
    """Outside everywhere but for a disc of `radius` points, one plane thick, in the last plane and its last rows: a small
    ball cut down to the points that the last workgroups own."""
    nu, nv, nw = shape
    v = np.full((nw, nv, nu), 1.0)
    j, i = np.indices((nv, nu))
    v[nw - 1][(i - nu // 2) ** 2 + (j - (nv - 2 - radius)) ** 2 < radius * radius] = -1.0
    return v


def row_ends(shape, last):
    """Inside everywhere but for the first (or the last) point of every row."""
    v = np.full((shape[2], shape[1], shape[0]), -1.0)
    v[:, :, -1 if last else 0] = 1.0
    return v


# ------------------------------------------------------------------------------------------------- what an input reaches

def chunk_labels(labels, n_records):
    """Per chunk of 64 consecutive points the smallest and the largest label that has a record (-1, -1: none)."""
    flat = np.asarray(labels).reshape(-1).astype(np.int64)
    flat = np.where((flat >= 0) & (flat < n_records), flat, -1)
    flat = np.append(flat, np.full(-len(flat) % WAVE, -1, np.int64)).reshape(-1, WAVE)
    high = flat.max(axis=1)
    low = np.where(flat >= 0, flat, np.iinfo(np.int64).max).min(axis=1)
    return np.where(high >= 0, low, -1), high


def wave_paths(labels, n_records, per_wave):
    """What parts_measure_kernel's waves meet, each over per_wave consecutive chunks: (carried, changed, mixed) -- pairs of
    successive chunks of one wave that hold the same single label, that hold two different single labels, and chunks with more
    than one label."""
    low, high = chunk_labels(labels, n_records)
    single = (low == high) & (low >= 0)
    at = np.arange(len(low) - 1)
    same_wave = at // per_wave == (at + 1) // per_wave
    pair = same_wave & single[:-1] & single[1:]
    return int((pair & (low[:-1] == low[1:])).sum()), int((pair & (low[:-1] != low[1:])).sum()), int((low != high).sum())
