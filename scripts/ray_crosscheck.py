"""Records tests/golden/ray_queries.npz: the reference's own Raymarcher.rayMarch + getNormal for a fixed set of caller-supplied
rays -- BUILD CONTAINER ONLY (it needs node and the reference sources, like scripts/ref_crosscheck.py).

The ray set (RAY_CATEGORIES) is generated with splitmix64 from a fixed seed and stored in the fixture with the results:
origins on the camera orbit, inside the BVH root box, inside a primitive, outside the +-10 octree cube; directions with
exact-zero components, unnormalised, and rays that point away from everything.  scripts/ref_crosscheck/rays.js marches
them through the reference's statements (type-stripped in memory, restated gl-matrix underneath: not a reference build, so
Mandelbulb [A] (preset 13) is left out -- node's Math.pow is not fdlibm's) for every configuration of configs().  The
fixture holds values the reference's programs produced (the rayMarch result as f64 bits, the Uint16Array counters, the
Float32Array normal as bits, whether the origin lies inside a primitive), nothing of the programs themselves.  The file is
written with fixed zip timestamps, so a second run gives the same bytes (tests/test_ray_queries.py).

usage: python scripts/ray_crosscheck.py [--out tests/golden/ray_queries.npz]"""
import argparse
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
RAYS_JS = os.path.join(ROOT, "scripts", "ref_crosscheck", "rays.js")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ray_queries.npz")
SEED = 0x52415953  # "RAYS"

RAY_CATEGORIES = ("orbit", "in_root_box", "in_primitive", "outside_cube", "zero_components", "unnormalised", "away")
ALGS = ("sphere-tracer", "fixed-step", "adaptive-step", "adaptive-step-v2", "adaptive-step-v3")
ACCELS = ("None", "Octree", "BVH")
SYNTHETIC_SPHERES = 1000


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & (2 ** 64 - 1)

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return z ^ (z >> 31)

    def uniform(self, lo, hi):
        return lo + (hi - lo) * ((self.next() >> 11) / float(1 << 53))

    def unit(self):
        while True:
            v = np.array([self.uniform(-1, 1) for _ in range(3)])
            n = float(np.sqrt((v * v).sum()))
            if 0.1 < n <= 1:
                return v / n


def ray_set():
    """(origins f32[n, 3], directions f32[n, 3], category u8[n]) -- deterministic."""
    r = SplitMix64(SEED)
    o, d, c = [], [], []

    def add(cat, org, dr):
        o.append(org)
        d.append(dr)
        c.append(RAY_CATEGORIES.index(cat))
    for _ in range(8):  # on the radius-3 camera orbit, looking roughly at the centre
        p = 3 * r.unit()
        add("orbit", p, -p / 3 + 0.3 * r.unit())
    for _ in range(12):  # inside the BVH root box of the presets (their objects sit within a few units of the origin)
        add("in_root_box", [r.uniform(-1.5, 1.5) for _ in range(3)], r.unit())
    add("in_primitive", [0, 0, 0], [0, 0, -1])
    for _ in range(5):  # at and next to the origin: inside the presets' central primitives
        add("in_primitive", [r.uniform(-0.1, 0.1) for _ in range(3)], r.unit())
    for _ in range(8):  # outside the +-10 octree cube (all-primitive fallback), heading inwards
        p = r.unit()
        p = p / np.abs(p).max() * r.uniform(10.5, 14)
        add("outside_cube", p, -p / np.linalg.norm(p) + 0.2 * r.unit())
    for k in range(10):  # exact-zero direction components: one or two axes
        v = r.unit()
        v[k % 3] = 0.0
        if k >= 6:
            v[(k + 1) % 3] = 0.0
        v = v / np.linalg.norm(v)
        org = [r.uniform(-4, 4) for _ in range(3)]
        if k % 2:
            org[k % 3] = 0.0  # and on the axis plane
        add("zero_components", org, v)
    for _ in range(10):  # unnormalised directions (rayMarch does not normalise)
        s = r.uniform(0.25, 4.0)
        add("unnormalised", [r.uniform(-5, 5) for _ in range(3)], r.unit() * s)
    for k in range(6):  # outside the cube pointing away from it
        axis = np.zeros(3)
        axis[k % 3] = 1.0 if k < 3 else -1.0
        add("away", axis * 12.5 + 0.5 * r.unit(), axis + 0.1 * r.unit())
    return (np.array(o, np.float64).astype(np.float32), np.array(d, np.float64).astype(np.float32), np.array(c, np.uint8))


def configs():
    """Every preset but Mandelbulb [A] (13) under the three structures; the five marchers on presets 0, 2, 3, 5, 17; a
    fixed step and V2 / V3 overshoots that are not the defaults; preset 12 at a non-zero time; 1 000 spheres, octree."""
    c = [dict(preset=p, accel=a, algorithm="sphere-tracer") for p in range(19) if p != 13 for a in ACCELS]
    c += [dict(preset=p, accel=a, algorithm=alg) for p in (0, 2, 3, 5, 17) for alg in ALGS[1:] for a in ACCELS]
    c += [dict(preset=3, accel=a, algorithm="fixed-step", stepSize=0.05) for a in ACCELS]
    c += [dict(preset=3, accel=a, algorithm="adaptive-step-v2", overshootFactor=1.5) for a in ACCELS]
    c += [dict(preset=3, accel=a, algorithm="adaptive-step-v3", overshootFactor=1.1) for a in ACCELS]
    c += [dict(preset=12, accel=a, algorithm="sphere-tracer", time=1.75) for a in ACCELS]
    c += [dict(synthetic=SYNTHETIC_SPHERES, accel="Octree", algorithm="sphere-tracer")]
    return c


def synthetic_spheres(n):
    sys.path.insert(0, ROOT)
    from cpu_raymarcher_amd.synthetic import synthetic_spheres as gen  # the C5 generator
    return gen(n)


def available():
    return os.path.isdir(REF) and shutil.which("node") is not None


def run_reference(origins, directions, cfgs, timeout=1800):
    job = {"origins": [float(v) for v in origins.reshape(-1)], "directions": [float(v) for v in directions.reshape(-1)], "configs": []}
    for cfg in cfgs:
        j = dict(cfg)
        if "synthetic" in j:
            j["spheres"] = [[float(v) for v in s] for s in synthetic_spheres(j.pop("synthetic"))]
        job["configs"].append(j)
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "rays.json")
        with open(p, "w") as f:
            json.dump(job, f)
        return json.loads(subprocess.check_output(["node", RAYS_JS, REF, p], timeout=timeout))


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same file bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            zi = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def record(path):
    o, d, cat = ray_set()
    cfgs = configs()
    res = run_reference(o, d, cfgs)
    write_npz(path, {
        "origins": o, "directions": d, "category": cat,
        "category_names": np.array(RAY_CATEGORIES), "configs": np.array(json.dumps(cfgs, sort_keys=True)),
        "t_bits": np.array([[int(x, 16) for x in r["t"]] for r in res], np.uint64),
        "sdf": np.array([r["sdf"] for r in res], np.uint16), "iters": np.array([r["iters"] for r in res], np.uint16),
        "normal_bits": np.array([r["normal"] for r in res], np.uint32).reshape(len(cfgs), -1, 3),
        "inside": np.array([r["inside"] for r in res], np.uint8),
    })


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    if not available():
        print("reference sources or node not present: nothing to record")
        return 0
    record(args.out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
