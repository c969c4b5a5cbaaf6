"""compareFrames of the N-API addon (native/rm_addon.cc) and FrameComparison of the JS host (native/host/raymarcher.js): typed
arrays through rm_compare_frames, against the Python result and the numpy model of tests/compare_model.py."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import compare_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
HAVE_HDR = os.path.exists("/usr/include/node/node_api.h")
pytestmark = pytest.mark.skipif(NODE is None or not HAVE_HDR, reason="node / node_api.h not present")

JS = r"""
const fs = require('fs'), path = require('path');
const [root, dir, W, rows, n, map, gain] = [process.argv[2], process.argv[3], +process.argv[4], +process.argv[5], +process.argv[6], process.argv[7], +process.argv[8]];
const host = require(path.join(root, 'native', 'host', 'raymarcher.js'));
function set(tag) {
  const u8 = (f) => new Uint8ClampedArray(fs.readFileSync(path.join(dir, f + tag + '.bin')));
  const u16 = (f) => { const b = fs.readFileSync(path.join(dir, f + tag + '.bin')); return new Uint16Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
  return { depth: u8('depth'), normal: u8('normal'), sdfEval: u16('sdf'), iters: u16('iters') };
}
const r = new host.FrameComparison(map, gain).compareFrames(set('_a'), set('_b'), W, rows, n);
if (r.rgba) fs.writeFileSync(path.join(dir, 'rgba.bin'), Buffer.from(r.rgba.buffer));
console.log(JSON.stringify(r.stats));
"""

CAMEL = {"pixels": "pixels", "sum_sdf_a": "sumSdfA", "sum_sdf_b": "sumSdfB", "sum_iters_a": "sumItersA", "sum_iters_b": "sumItersB",
         "sum_abs_depth": "sumAbsDepth", "surface_a": "surfaceA", "surface_b": "surfaceB", "surface_only_a": "surfaceOnlyA",
         "surface_only_b": "surfaceOnlyB", "depth_differs": "depthDiffers", "normal_differs": "normalDiffers",
         "counters_differ": "countersDiffer", "b_cheaper": "bCheaper", "a_cheaper": "aCheaper", "max_abs_depth": "maxAbsDepth",
         "max_abs_normal": "maxAbsNormal"}


@pytest.fixture(scope="module")
def addon(rm):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "native")])
    return os.path.join(ROOT, "native", "build", "rm_addon.node")


def test_host_only_context_refuses_to_compare(addon):
    js = ("const a=require(%r);a.create(-1);const s={depth:new Uint8ClampedArray(4)};"
          "console.log(a.compareFrames(s,s,2,2,1,2,5,new Uint8ClampedArray(16),new Uint8Array(128)),"
          "a.compareFrames(s,s,2,2,1,0,5,new Uint8ClampedArray(16),null),a.compareFrames(s,s,2,2,1,2,5,new Uint8ClampedArray(8),null))" % addon)
    out = subprocess.check_output([NODE, "-e", js]).decode().split()
    assert out == ["-3", "-1", "-1"]  # no device; the map's buffer is absent; the image buffer is too small


@pytest.mark.gpu
@pytest.mark.parametrize("map,gain", [("sdf", 5), ("surface", 1), ("none", 5)])
def test_compare_frames_equals_python(addon, rm, tmp_path, map, gain):
    W, rows, n = 33, 9, 3
    total = W * rows * n
    rng = np.random.default_rng(4)
    sets = []
    for tag in ("_a", "_b"):
        s = (rng.integers(0, 256, total, dtype=np.uint8), rng.integers(126, 131, 3 * total, dtype=np.uint8),
             rng.integers(0, 65536, total, dtype=np.uint16), rng.integers(0, 9, total, dtype=np.uint16))
        s[1][np.repeat(rng.random(total) < 0.4, 3)] = 128
        for name, x in zip(("depth", "normal", "sdf", "iters"), s):
            x.tofile(str(tmp_path / (name + tag + ".bin")))
        sets.append(s)
    (tmp_path / "run.js").write_text(JS)
    out = subprocess.check_output([NODE, str(tmp_path / "run.js"), ROOT, str(tmp_path), str(W), str(rows), str(n), map, str(gain)])
    got = [{k: r[v] for k, v in CAMEL.items()} for r in json.loads(out)]
    ctx = rm.Context(0)
    rgba = np.zeros(4 * total, np.uint8)
    stats = np.zeros(128 * n, np.uint8)
    ctx.compare_frames(sets[0], sets[1], rgba=rgba if map != "none" else None, map=map, gain=gain, stats=stats, width=W, rows=rows, n_frames=n)
    want, img = M.compare_frames(sets[0], sets[1], W * rows, n, M.MAPS[map], gain)
    assert got == ctx.decode_compare_stats(stats) == want
    if map != "none":
        js_rgba = np.fromfile(str(tmp_path / "rgba.bin"), dtype=np.uint8)
        assert np.array_equal(js_rgba, rgba) and np.array_equal(rgba, img)
    ctx.close()
