"""The reference's own TypeScript control flow -- type syntax removed in memory, a restated gl-matrix underneath -- must
produce the oracle's bytes (scripts/ref_crosscheck.py).  What that flow produced (SHA-256 of the five buffers and the
counter sums per configuration, nothing else) is recorded in tests/golden/ref_crosscheck.json by
`scripts/ref_crosscheck.py --quick --record tests/golden/ref_crosscheck.json`, so these tests need neither node nor the
reference sources.  Not a reference build; it does not pin parity, it guards the oracle's reading of
bvh.ts / octree.ts / scene.ts / the marchers against misreadings."""
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "ref_crosscheck.py")
RECORDED = os.path.join(ROOT, "tests", "golden", "ref_crosscheck.json")


def test_reference_control_flow_matches_the_oracle():
    p = subprocess.run([sys.executable, SCRIPT, "--quick", "--recorded", RECORDED], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=1500)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "8 configurations, 0 differ" in out, out


def test_type_stripper_leaves_no_type_syntax(oracle):
    """Every module of the render path compiled after stripping (run.js exits 3 otherwise) for each marcher and shader,
    built the scene, and rendered what the oracle renders."""
    spec = importlib.util.spec_from_file_location("ref_crosscheck", SCRIPT)
    rc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rc)
    with open(RECORDED) as f:
        recorded = json.load(f)["stripper"]
    assert len(rc.STRIPPER_CASES) == 4
    for name, cfg in rc.STRIPPER_CASES:
        rec = recorded[name]
        assert rec["config"] == cfg, name
        ref = rec["reference"]
        assert ref["n_objects"] > 0, name
        orc = rc.oracle_flow(oracle, cfg)
        assert orc["sha256"] == ref["sha256"], name
        assert all(orc[k] == ref[k] for k in ("total_sdf", "total_iters", "max_sdf", "min_sdf")), name
