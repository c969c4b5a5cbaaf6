'use strict';
/*
 * JS host mirror of the reference's plugin surface for the render path, on top of the N-API
 * addon (native/rm_addon.cc -> include/rm_raymarch.h).  Same class and method names, argument
 * order and defaulting as the TypeScript (paths relative to the reference's src/):
 *
 *   Scene(accelerationStructure)            util/scene.ts:24-59
 *   Camera.setAngles / rotateCamera         util/camera.ts:27-62
 *   SphereTracer.runRaymarcher(...)         cpu_algorithms/raymarcher.ts:46-57
 *   createShadingModelFromValue(name)       main.ts:33-45
 *   onmessage(job) -> Result                workers/raymarchWorker.ts:33-92
 *
 * Buffers are the reference's typed arrays.  RM_E_UNSUPPORTED (-2) surfaces as an Error with
 * .code === -2 so a host can keep its TypeScript CPU path for that job.
 */
const path = require('path');
const native = require(path.join(__dirname, '..', 'build', 'rm_addon.node'));

const RM_SCENE_UPLOADED = -2147483648; // include/rm_raymarch.h: the scene last uploaded or edited

let created = false;
function ensure(device) {
  if (!created) {
    const rc = native.create(device === undefined ? 0 : device);
    if (rc !== 0) { const e = new Error('rm_create failed (' + rc + '): no usable HIP device'); e.code = rc; throw e; }
    created = true;
  }
}
function check(rc) {
  if (rc === 0) return;
  const e = new Error(native.lastError() + ' (' + rc + ')');
  e.code = rc;
  throw e;
}

class Camera { // util/camera.ts
  constructor() { this.pitch = 0; this.yaw = 0; }
  setAngles(pitch, yaw) { this.pitch = Math.min(Math.max(pitch, -Math.PI / 2), Math.PI / 2); this.yaw = yaw; }
  rotateCamera(pitch, yaw) { this.pitch = Math.min(Math.max(this.pitch + pitch, -Math.PI / 2), Math.PI / 2); this.yaw += yaw; }
  getAngles() { return [this.pitch, this.yaw]; }
}

class Scene { // util/scene.ts
  constructor(accelerationStructure = 'None') {
    ensure();
    this.accelerationStructure = accelerationStructure;
    this.camera = new Camera();
    this.currentPresetIndex = 0;
  }
  loadPreset(index) { this.currentPresetIndex = Math.max(0, Math.min(index, 18)); }
  // Object CRUD on sphere scenes (the reference README's third plan; rm_scene_edit_spheres): edits is a list of
  // { op: 'set' | 'insert' | 'remove', index, center: [x, y, z], radius } applied in order to the scene's sphere list, indices in
  // object order at the moment each edit applies.  The scene (preset 0..4, or one edited before) is the uploaded scene
  // afterwards: jobs select it with scenePresetIndex = RM_SCENE_UPLOADED, which currentPresetIndex then holds.  All or nothing.
  editSpheres(edits) {
    const ops = new Int32Array(2 * edits.length), spheres = new Float64Array(4 * edits.length);
    edits.forEach((e, i) => {
      ops[2 * i] = { set: 0, insert: 1, remove: 2 }[e.op];
      ops[2 * i + 1] = e.index;
      spheres.set([...(e.center || [0, 0, 0]), e.radius === undefined ? 0 : e.radius], 4 * i);
    });
    check(native.editSpheres(this.currentPresetIndex, this.accelerationStructure, ops, spheres));
    if (edits.length) this.currentPresetIndex = RM_SCENE_UPLOADED;
  }
  setSphere(index, center, radius) { this.editSpheres([{ op: 'set', index, center, radius }]); }
  insertSphere(index, center, radius) { this.editSpheres([{ op: 'insert', index, center, radius }]); }
  removeSphere(index) { this.editSpheres([{ op: 'remove', index }]); }
}

class Raymarcher { // cpu_algorithms/raymarcher.ts:19-57
  constructor() { this.algorithm = 'sphere-tracer'; }
  getMaxDistance() { return 10; }
  runRaymarcher(scene, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer, width, height, time,
    yStart = 0, yEnd = height) {
    check(native.renderTile({
      width, height, time, yStart, yEnd, camera: { pitch: scene.camera.pitch, yaw: scene.camera.yaw },
      algorithm: this.algorithm, scenePresetIndex: scene.currentPresetIndex,
      accelerationStructure: scene.accelerationStructure, overshootFactor: this.overshootFactor, stepSize: this.stepSize,
    }, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer));
  }
}
class SphereTracer extends Raymarcher {}
class FixedStep extends Raymarcher { constructor(stepSize) { super(); this.algorithm = 'fixed-step'; this.stepSize = stepSize; } }
class AdaptiveStep extends Raymarcher { constructor() { super(); this.algorithm = 'adaptive-step'; } }
class AdaptiveStepV2 extends Raymarcher { constructor(o) { super(); this.algorithm = 'adaptive-step-v2'; this.overshootFactor = o; } }
class AdaptiveStepV3 extends Raymarcher { constructor(o) { super(); this.algorithm = 'adaptive-step-v3'; this.overshootFactor = o; } }

class ShadingModel { // util/shading_models/shadingModel.ts:8-17
  constructor(name) { this.name = name || 'normal'; }
  shade(shadedBuffer, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer, width, height) {
    ensure();
    check(native.shade(this.name, width, height, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer, shadedBuffer));
    return shadedBuffer;
  }
}
function createShadingModelFromValue(selectedModel) { // main.ts:33-45
  return new ShadingModel(['phong', 'sdf-heatmap', 'iteration-heatmap'].includes(selectedModel) ? selectedModel : 'normal');
}

function onmessage(job) { // workers/raymarchWorker.ts:33-92
  const scene = new Scene(job.accelerationStructure);
  scene.loadPreset(job.scenePresetIndex);
  scene.camera.setAngles(job.camera.pitch, job.camera.yaw);
  const tileHeight = Math.max(0, job.yEnd - job.yStart);
  const depth = new Uint8ClampedArray(job.width * tileHeight);
  const normal = new Uint8ClampedArray(job.width * tileHeight * 3);
  const sdfEval = new Uint16Array(job.width * tileHeight);
  const iters = new Uint16Array(job.width * tileHeight);
  let alg;
  switch (job.algorithm) {
    case 'fixed-step': alg = new FixedStep(job.stepSize); break;
    case 'adaptive-step': alg = new AdaptiveStep(); break;
    case 'adaptive-step-v2': alg = new AdaptiveStepV2(job.overshootFactor); break;
    case 'adaptive-step-v3': alg = new AdaptiveStepV3(job.overshootFactor); break;
    default: alg = new SphereTracer();
  }
  alg.runRaymarcher(scene, depth, normal, sdfEval, iters, job.width, job.height, job.time, job.yStart, job.yEnd);
  return { yStart: job.yStart, yEnd: job.yEnd, depth, normal, sdfEval, iters };
}

function diagnostics(SDFevaluationBuffer, iterationsBuffer) { // main.ts:528-548
  ensure();
  const d = native.diagnostics(SDFevaluationBuffer, iterationsBuffer);
  if (typeof d === 'number') check(d);
  d.averageSDFCalls = d.totalSDFCalls / Math.max(1, d.totalPixels);
  d.averageIterations = d.totalIterations / Math.max(1, d.totalPixels);
  return d;
}

// Two G-buffer sets of the same frames, B against A (rm_compare_frames): the analytics the reference's README plans
// ("comparing different algorithms").  Sets are {depth, normal, sdfEval, iters} as onmessage returns them (a buffer may be
// absent on both sides); nFrames frames lie one behind the other.
const COMPARE_MAPS = { none: -1, sdf: 0, iters: 1, depth: 2, normal: 3, surface: 4 };
const COMPARE_FIELDS = ['pixels', 'sumSdfA', 'sumSdfB', 'sumItersA', 'sumItersB', 'sumAbsDepth', 'surfaceA', 'surfaceB',
  'surfaceOnlyA', 'surfaceOnlyB', 'depthDiffers', 'normalDiffers', 'countersDiffer', 'bCheaper', 'aCheaper'];
class FrameComparison {
  constructor(map = 'sdf', gain = 5) { this.map = map; this.gain = gain; }
  // -> { stats: one object per frame, rgba: Uint8ClampedArray | null }
  compareFrames(a, b, width, rows, nFrames = 1) {
    ensure();
    const map = typeof this.map === 'number' ? this.map : COMPARE_MAPS[this.map];
    const rgba = map === -1 ? null : new Uint8ClampedArray(width * rows * nFrames * 4);
    const raw = new Uint8Array(128 * nFrames);
    check(native.compareFrames(a, b, width, rows, nFrames, map, this.gain, rgba, raw));
    const view = new DataView(raw.buffer);
    const stats = [];
    for (let k = 0; k < nFrames; k++) {
      const s = {};
      COMPARE_FIELDS.forEach((name, i) => { s[name] = Number(view.getBigUint64(128 * k + 8 * i, true)); });
      s.maxAbsDepth = view.getUint32(128 * k + 120, true);
      s.maxAbsNormal = view.getUint32(128 * k + 124, true);
      stats.push(s);
    }
    return { stats, rgba };
  }
}

module.exports = { Camera, Scene, Raymarcher, SphereTracer, FixedStep, AdaptiveStep, AdaptiveStepV2, AdaptiveStepV3,
  ShadingModel, createShadingModelFromValue, onmessage, diagnostics, FrameComparison, native };
