'use strict';
/*
 * rays.js -- the reference's own Raymarcher.rayMarch + getNormal for caller-supplied rays.  BUILD CONTAINER ONLY.
 *
 * The same loading as run.js: the reference's TypeScript sources are read as TEXT at run time from the directory given on
 * the command line (never copied, never written anywhere), type syntax is removed in memory (strip_ts.js) and `gl-matrix`
 * resolves to the restated glmatrix_shim.js.  For every configuration it builds the scene the way the worker does
 * (new Scene(accel), loadPreset; or SceneManager.createSphere for an uploaded sphere list), calls scene.updateTime(time), and
 * per ray i calls the marcher's rayMarch(scene, origin, direction, i, sdf, iters) and, unless the distance reaches
 * getMaxDistance(), getNormal(scene, hitPosition, i, sdf) at hitPosition = scaleAndAdd(origin, direction, depth) -- the
 * statements of raymarcher.ts:89-102 with the ray supplied instead of generated.  It also records whether
 * Scene.getDistance(origin) < 0 (the origin lies inside a primitive).
 *
 * It prints only output values, as JSON on stdout: per configuration the rayMarch result as IEEE-754 bit patterns (hex),
 * the Uint16Array counters, the Float32Array normal as bit patterns and the inside flags.
 *
 * usage: node rays.js <reference src dir> <input.json>
 *   input: {origins: [x, y, z, ...], directions: [...], configs: [{preset | spheres: [[x, y, z, r], ...], accel, algorithm,
 *           overshootFactor?, stepSize?, time?}, ...]}
 */
const fs = require('fs');
const path = require('path');
const vm = require('vm');
const { strip } = require('./strip_ts.js');
const shim = require('./glmatrix_shim.js');

const SRC = path.resolve(process.argv[2]);
const input = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const cache = new Map();

function load(absNoExt) {  // as run.js
  const file = absNoExt.endsWith('.ts') ? absNoExt : absNoExt + '.ts';
  if (cache.has(file)) return cache.get(file);
  const exports_ = {};
  cache.set(file, exports_);
  const text = fs.readFileSync(file, 'utf8');
  const js = strip(text, path.relative(SRC, file));
  const require_ = (spec) => {
    if (spec === 'gl-matrix') return shim;
    if (spec.startsWith('.')) return load(path.resolve(path.dirname(file), spec));
    throw new Error('module ' + spec + ' is not on the render path (imported by ' + file + ')');
  };
  const fn = new vm.Script('(function (require_, exports_) {"use strict";\n' + js + '\n})', { filename: 'stripped:' + path.relative(SRC, file) }).runInThisContext();
  fn(require_, exports_);
  return exports_;
}

const { vec3 } = shim;
const { Scene } = load(path.join(SRC, 'util', 'scene'));
const { SceneManager } = load(path.join(SRC, 'util', 'sceneManager'));
const algs = {
  'sphere-tracer': (c) => new (load(path.join(SRC, 'cpu_algorithms', 'sphereTracer')).SphereTracer)(),
  'fixed-step': (c) => new (load(path.join(SRC, 'cpu_algorithms', 'fixedStep')).FixedStep)(c.stepSize),
  'adaptive-step': (c) => new (load(path.join(SRC, 'cpu_algorithms', 'adaptiveStep')).AdaptiveStep)(),
  'adaptive-step-v2': (c) => new (load(path.join(SRC, 'cpu_algorithms', 'adaptiveStepV2')).AdaptiveStepV2)(c.overshootFactor),
  'adaptive-step-v3': (c) => new (load(path.join(SRC, 'cpu_algorithms', 'adaptiveStepV3')).AdaptiveStepV3)(c.overshootFactor),
};

const n = input.origins.length / 3;
const f64 = new Float64Array(1), u64 = new BigUint64Array(f64.buffer);
const out = [];
for (const cfg of input.configs) {
  const scene = new Scene(cfg.accel);
  if (cfg.spheres) {  // an uploaded sphere list: the scene's objects replaced, its structure rebuilt (scene.ts:38-59)
    scene.objectSDFs = cfg.spheres.map((s) => SceneManager.createSphere(s[0], s[1], s[2], s[3]));
    scene.cachedBounds = null;
    if (cfg.accel === 'Octree') scene.buildOctree();
    else if (cfg.accel === 'BVH') scene.buildBVH();
  } else {
    scene.loadPreset(cfg.preset);
  }
  scene.updateTime(cfg.time || 0);
  const alg = (algs[cfg.algorithm] || algs['sphere-tracer'])(cfg);
  const MAX_DIST = alg.getMaxDistance();
  const sdf = new Uint16Array(n), iters = new Uint16Array(n);
  const t = [], normal = new Float32Array(3 * n), inside = [];
  for (let i = 0; i < n; i++) {
    const o = vec3.fromValues(input.origins[3 * i], input.origins[3 * i + 1], input.origins[3 * i + 2]);
    const d = vec3.fromValues(input.directions[3 * i], input.directions[3 * i + 1], input.directions[3 * i + 2]);
    inside.push(scene.getDistance(o) < 0 ? 1 : 0);
    const depth = alg.rayMarch(scene, o, d, i, sdf, iters);
    const hit = vec3.create();
    vec3.scaleAndAdd(hit, o, d, depth);
    const nrm = depth >= MAX_DIST ? vec3.fromValues(0, 0, 0) : alg.getNormal(scene, hit, i, sdf);
    normal[3 * i] = nrm[0];
    normal[3 * i + 1] = nrm[1];
    normal[3 * i + 2] = nrm[2];
    f64[0] = depth;
    t.push(u64[0].toString(16));
  }
  out.push({ t, sdf: Array.from(sdf), iters: Array.from(iters), normal: Array.from(new Uint32Array(normal.buffer)), inside });
}
process.stdout.write(JSON.stringify(out) + '\n');
