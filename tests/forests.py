"""Seeded, deterministic expression forests in the oracle's `prims` format (nested dicts; OracleScene(prims=...)): the random
generators the parity tests have always used, and the LIMIT forests of test_rtc_limits.py -- one member just inside and one
just outside every limit the product names for an uploaded forest:

  rm_rtc.h          32 objects, 512 instructions for a scene kernel compiled at run time (beyond: the interpreter)
  rm_rtc.cpp        emit_bvh: the BVH becomes code up to 8 non-empty leaves, finite nested boxes
  rm_types.h        RM_PROG_MAX_SLOTS / RM_PROG_MAX_VALS: 16 position slots, 16 pending values in the interpreter
  rm_scene_host.cpp (slots * 12 + values * 8) * 256 <= 64 KiB of LDS for the interpreter's stacks (beyond: RM_E_UNSUPPORTED)

and forests that put the run-time compiled kernels under register pressure.  Which side of its limit a forest lands on is
asserted by test_rtc_limits.py from what the library reports, so a change of a limit or of this file cannot pass silently."""
import numpy as np


def random_forest(rng, n_roots):
    """Nested dicts in the oracle's prims format: random operator trees over random leaves."""
    def leaf():
        kind = rng.choice(["sphere", "box", "torus"])
        d = {"type": str(kind), "pos": [float(np.float32(v)) for v in rng.uniform(-1.2, 1.2, 3)],
             "rot": [float(np.float32(v)) for v in rng.uniform(-3, 3, 3)] if rng.random() < 0.5 else None}
        if kind == "sphere":
            d["r"] = float(rng.uniform(0.1, 0.4))
        elif kind == "box":
            d["half"] = [float(np.float32(v)) for v in rng.uniform(0.05, 0.35, 3)]
        else:
            d["radius"] = float(rng.uniform(0.15, 0.4))
        return d

    def tree(depth):
        if depth == 0 or rng.random() < 0.25:
            return leaf()
        op = rng.choice(["round", "smoothUnion", "smoothSub", "twist", "anim", "repetition"],
                        p=[0.25, 0.3, 0.15, 0.15, 0.1, 0.05])
        if op == "round":
            return {"type": "round", "a": tree(depth - 1), "radius": float(rng.uniform(0.01, 0.15))}
        if op == "twist":
            return {"type": "twist", "a": tree(depth - 1), "amount": float(rng.uniform(0.5, 4))}
        if op == "anim":
            return {"type": "anim", "a": tree(depth - 1), "direction": [float(v) for v in rng.uniform(-1, 1, 3)],
                    "amplitude": float(rng.uniform(0.1, 0.6)), "speed": float(rng.uniform(0.001, 0.01))}
        if op == "repetition":
            return {"type": "repetition", "a": tree(depth - 1), "spacing": [float(np.float32(v)) for v in rng.uniform(2.5, 4, 3)]}
        return {"type": str(op), "a": tree(depth - 1), "b": tree(depth - 1), "k": float(rng.uniform(0.01, 0.3))}

    return [tree(4) for _ in range(n_roots)]


def plain_forest(rng, n_roots, depth, k_range):
    """Spheres, boxes and tori (half of them rotated) under Round / SmoothUnion / SmoothSubtraction only: the trees whose
    specialised code prunes operands by binary32 intervals (csrc/rm_rtc.cpp)."""
    def leaf():
        kind = rng.choice(["sphere", "box", "torus"], p=[0.3, 0.5, 0.2])
        d = {"type": str(kind), "pos": [float(np.float32(v)) for v in rng.uniform(-0.9, 0.9, 3)],
             "rot": [float(np.float32(v)) for v in rng.uniform(-3, 3, 3)] if rng.random() < 0.5 else None}
        if kind == "sphere":
            d["r"] = float(rng.uniform(0.1, 0.4))
        elif kind == "box":
            d["half"] = [float(np.float32(v)) for v in rng.uniform(0.02, 0.4, 3)]
        else:
            d["radius"] = float(rng.uniform(0.15, 0.4))
        return d

    def tree(dep):
        if dep == 0 or (dep < depth and rng.random() < 0.15):
            return leaf()
        op = rng.choice(["round", "smoothUnion", "smoothSub"], p=[0.2, 0.6, 0.2]) if dep < depth else "smoothUnion"
        if op == "round":
            return {"type": "round", "a": tree(dep - 1), "radius": float(rng.uniform(0.005, 0.1))}
        return {"type": str(op), "a": tree(dep - 1), "b": tree(dep - 1), "k": float(np.exp(rng.uniform(*np.log(k_range))))}

    return [tree(depth) for _ in range(n_roots)]


# ---------------------------------------------------------------------------------------------------------- limit forests

def _sphere(x, y, z, r, rot=None):
    return {"type": "sphere", "pos": [float(np.float32(x)), float(np.float32(y)), float(np.float32(z))], "rot": rot, "r": float(r)}


def _box(x, y, z, h, rot=None):
    return {"type": "box", "pos": [float(np.float32(x)), float(np.float32(y)), float(np.float32(z))], "rot": rot,
            "half": [float(np.float32(v)) for v in h]}


def _torus(x, y, z, radius, rot=None):
    return {"type": "torus", "pos": [float(np.float32(x)), float(np.float32(y)), float(np.float32(z))], "rot": rot, "radius": float(radius)}


def _round(a, radius):
    return {"type": "round", "a": a, "radius": float(radius)}


def _twist(a, amount):
    return {"type": "twist", "a": a, "amount": float(amount)}


def _union(a, b, k):
    return {"type": "smoothUnion", "a": a, "b": b, "k": float(k)}


def _grid(k):
    """Object k's place on a 4 x 4 x 3 lattice inside the camera's view."""
    return 0.55 * (k % 4) - 0.825, 0.55 * ((k // 4) % 4) - 0.825, 0.5 * (k // 16) - 0.5


def many_objects(n):
    """n objects, single leaves and small trees in turn (the object limit of a scene kernel is 32)."""
    out = []
    for k in range(n):
        x, y, z = _grid(k)
        rot = [0.3 * k, 0.1 * k, -0.2 * k] if k % 3 == 0 else None
        kind = k % 5
        if kind == 0:
            out.append(_sphere(x, y, z, 0.12 + 0.002 * k))
        elif kind == 1:
            out.append(_box(x, y, z, (0.1, 0.14, 0.08), rot))
        elif kind == 2:
            out.append(_round(_box(x, y, z, (0.08, 0.08, 0.12), rot), 0.04))
        elif kind == 3:
            out.append(_torus(x, y, z, 0.16, rot))
        else:
            out.append(_union(_sphere(x, y, z, 0.11), _box(x, y + 0.1, z, (0.12, 0.03, 0.12)), 0.05))
    return out


def round_chain(leaf, n_rounds):
    """n_rounds Rounds around one leaf: 1 + 2 * n_rounds instructions (PRE and POST half of every Round) and n_rounds + 1
    position slots."""
    for k in range(n_rounds):
        leaf = _round(leaf, 0.001 + 0.0005 * (k % 7))
    return leaf


def instruction_forest(total):
    """`total` interpreter instructions (the limit of a scene kernel is 512) in objects of 27: chains of thirteen Rounds over
    a sphere or a box, and a shorter chain or a lone leaf for the remainder."""
    out = []
    while total > 0:
        k = len(out)
        x, y, z = _grid(k)
        n = min(27, total)
        n -= 1 - n % 2  # (a chain has an odd number of instructions)
        leaf = _sphere(x, y, z, 0.1) if k % 2 else _box(x, y, z, (0.09, 0.07, 0.1), [0.2 * k, 0.0, 0.1 * k])
        out.append(round_chain(leaf, (n - 1) // 2))
        total -= n
    return out


def row_of_objects(n, spacing=0.45):
    """n well separated small objects on a diagonal line: the BVH builder's leaves are then decided by n alone."""
    out = []
    for k in range(n):
        t = (k - (n - 1) / 2) * spacing
        out.append(_sphere(t, 0.3 * t, -0.2 * t, 0.1) if k % 2 else _round(_box(t, 0.3 * t, -0.2 * t, (0.08, 0.1, 0.06), [0.0, 0.4 * k, 0.0]), 0.02))
    return out


def repetition_among_many():
    """A Repetition (infinite bounding box: the tree stays data) among eleven finite objects."""
    out = row_of_objects(11, 0.3)
    out.insert(5, {"type": "repetition", "a": _sphere(0.0, 0.0, 0.0, 0.15), "spacing": [3.0, 3.5, 3.0]})
    return out


def coincident_objects():
    """Objects whose bounding boxes are identical bit for bit (the nesting check of emit_bvh at equality): four copies of one
    sphere, three of one rounded box, and two unlike objects that share a box, beside two ordinary ones."""
    s = lambda: _sphere(0.3, 0.2, -0.1, 0.25)  # noqa: E731
    b = lambda: _round(_box(-0.5, -0.3, 0.2, (0.2, 0.15, 0.1)), 0.05)  # noqa: E731
    return [s(), b(), s(), _sphere(-0.4, 0.5, 0.0, 0.2), _box(-0.4, 0.5, 0.0, (0.2, 0.2, 0.2)), s(), b(), _torus(0.6, -0.5, 0.3, 0.2, [0.5, 0.2, 0.0]),
            b(), s(), _sphere(0.0, -0.7, -0.4, 0.15)]


def slot_chain(depth):
    """One object whose deepest leaf reads position slot `depth`: a Twist at either end and Rounds between (an operator above
    a Twist keeps its PRE half, so every level takes a slot).  The interpreter then needs depth + 1 slots."""
    t = _twist(_box(0.0, 0.0, 0.0, (0.3, 0.5, 0.2), [0.3, 0.2, 0.1]), 1.5)
    for k in range(depth - 2):
        t = _round(t, 0.002 + 0.001 * (k % 3))
    return _twist(t, 0.7)


def value_chain(n_leaves, x0=0.0):
    """One object of n_leaves leaves under SmoothUnions nested in the SECOND operand: every first operand waits for the rest
    of the chain, so the interpreter holds n_leaves pending values at the innermost leaf (nested in the first operand the
    chain would need two)."""
    def leaf(k):
        a = 0.9 * k
        x, y, z = x0 + 0.55 * np.cos(a) * (0.3 + 0.05 * k), 0.55 * np.sin(a) * (0.3 + 0.05 * k), 0.08 * k - 0.5
        return _sphere(x, y, z, 0.16) if k % 3 else _box(x, y, z, (0.12, 0.1, 0.14), [0.1 * k, 0.3, 0.0])
    t = leaf(n_leaves - 1)
    for k in reversed(range(n_leaves - 1)):
        t = _union(leaf(k), t, 0.03 + 0.01 * (k % 4))
    return t


def lds_forest(slots, vals):
    """Two objects: one that needs `slots` position slots, one that needs `vals` pending values.  The interpreter's stacks
    take (slots * 12 + vals * 8) bytes of LDS per lane."""
    return [slot_chain(slots - 1), value_chain(vals)]


def every_operator():
    """Twist, AnimatedTranslate, Repetition, SmoothSubtraction, Round and SmoothUnion over every leaf type, the Mandelbulb
    among them."""
    bulb = {"type": "mandelbulb", "pos": [0.6, 0.5, 0.0], "rot": None, "power": 8.0, "iterations": 6, "animate": True, "speed": 0.0002}
    anim = {"type": "anim", "a": _torus(0.0, 0.0, 0.0, 0.25, [1.2, 0.0, 0.3]), "direction": [0.3, 1.0, -0.2], "amplitude": 0.3, "speed": 0.004}
    sub = {"type": "smoothSub", "a": _round(_box(-0.6, -0.4, 0.0, (0.3, 0.3, 0.3), [0.0, 0.7, 0.0]), 0.05), "b": _sphere(-0.6, -0.4, 0.0, 0.33), "k": 0.08}
    rep = {"type": "repetition", "a": _round(_sphere(0.0, 0.0, 0.0, 0.08), 0.01), "spacing": [2.6, 3.0, 2.8]}
    return [_union(_twist(_box(-0.5, 0.5, 0.1, (0.15, 0.35, 0.15)), 2.5), anim, 0.1), sub, rep, {"type": "round", "a": bulb, "radius": 0.01}]


def limit_forests():
    """name -> forest, in a fixed order.  The names are what test_rtc_limits.py lists its expectations and its compile
    assignment under; `*_out` members lie beyond their limit."""
    return {
        "objects_31": many_objects(31),
        "objects_32": many_objects(32),
        "objects_33_out": many_objects(33),
        "instructions_512": instruction_forest(512),
        "instructions_513_out": instruction_forest(513),
        "bvh_leaves_8": row_of_objects(BVH_8_LEAVES),
        "bvh_leaves_9_out": row_of_objects(BVH_9_LEAVES),
        "repetition_among_many": repetition_among_many(),
        "coincident": coincident_objects(),
        "slots_15": [slot_chain(14)],
        "slots_16_out": [slot_chain(15)],
        "values_16": [value_chain(16)],
        "values_17_out": [value_chain(17)],
        "lds_exact": lds_forest(12, 14),       # (12 * 12 + 14 * 8) * 256 == 65536
        "lds_under": lds_forest(12, 13),
        "lds_over_out": lds_forest(12, 15),
        "random_8": random_forest(np.random.default_rng(101), 8),
        "random_16": random_forest(np.random.default_rng(102), 16),
        "random_30": random_forest(np.random.default_rng(103), 30),
        "plain_depth_6": plain_forest(np.random.default_rng(104), 1, 6, (1e-4, 0.05)),
        "every_operator": every_operator(),
    }


# objects on row_of_objects' line that give the BVH exactly eight / nine non-empty leaves (asserted from rm_scene_get_info)
BVH_8_LEAVES, BVH_9_LEAVES = 16, 17
