"""Host-side mirror of the reference's plugin surface for the render path, on top of the C ABI.

Same names, argument meaning and defaulting as the TypeScript (paths relative to the
reference's src/), so parity tests read like the reference's call sites:

  Scene(accelerationStructure)        util/scene.ts:24-59      loadPreset, camera, getDistance
  Camera.setAngles / rotateCamera     util/camera.ts:27-62
  SphereTracer().runRaymarcher(...)   cpu_algorithms/raymarcher.ts:46-57
  createShadingModelFromValue(name)   main.ts:33-45  -> NormalModel | PhongModel | SDFHeatmap | IterationHeatmap
  ShadingModel.shade(...)             util/shading_models/shadingModel.ts:8-17
  Job / Result / onmessage            workers/raymarchWorker.ts:10-92
  renderFrame (fan-out / fan-in)      main.ts:444-468,493-501
  diagnostics                         main.ts:528-548

Buffers are numpy arrays (host entry points) or torch CUDA tensors (device entry points,
asynchronous on torch's current stream).
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _native as N
from .context import Context, _is_torch, camera_rays, partition_rows, percentile  # noqa: F401

ALGORITHMS = ("sphere-tracer", "fixed-step", "adaptive-step", "adaptive-step-v2", "adaptive-step-v3")
SHADERS = ("normal", "phong", "sdf-heatmap", "iteration-heatmap")


class Camera:
    """util/camera.ts: orbit camera; the matrices themselves are derived inside the library."""

    def __init__(self):
        self.pitch = 0.0
        self.yaw = 0.0

    def setAngles(self, pitch, yaw):  # camera.ts:58-62
        self.pitch = min(max(pitch, -math.pi / 2), math.pi / 2)
        self.yaw = yaw

    def rotateCamera(self, pitch, yaw):  # camera.ts:27-32
        self.pitch = min(max(self.pitch + pitch, -math.pi / 2), math.pi / 2)
        self.yaw += yaw

    def getAngles(self):  # camera.ts:35-37
        return [self.pitch, self.yaw]


class Scene:
    """util/scene.ts Scene: primitives + camera + chosen acceleration structure.  The built
    structure lives in HBM inside `ctx`; loadPreset(i) rebuilds only on change."""

    def __init__(self, accelerationStructure="None", ctx: Optional[Context] = None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.accelerationStructure = accelerationStructure
        self.camera = Camera()
        self._uploaded = False
        self._session = None  # the open MeshSession (meshSession); every load of another scene closes it
        self.currentPresetIndex = 0
        self.time = 0.0  # Scene.updateTime's value (scene.ts:135-140): what rayMarch / getNormal march with
        self.loadPreset(0)  # scene.ts:28

    @property
    def accel_enum(self):
        return N.lib().rm_accel_from_string(str(self.accelerationStructure).encode())

    def loadPreset(self, index):  # scene.ts:38-59
        count = N.lib().rm_preset_count()
        self.currentPresetIndex = max(0, min(int(index), count - 1))
        self._uploaded = False
        self._session = None
        self.ctx.scene_from_preset(self.currentPresetIndex, self.accel_enum)

    def loadSpheres(self, centers, radii):
        """Build-defined: n spheres as SceneManager.createSphere(x,y,z,r) makes them."""
        self.ctx.scene_from_spheres(centers, radii, self.accel_enum)
        self._uploaded = True
        self._session = None

    def loadPrims(self, prims):
        """Build-defined: spheres / boxes / tori as (type, world_to_local[16], params)."""
        self.ctx.scene_from_prims(prims, self.accel_enum)
        self._uploaded = True
        self._session = None

    def loadNodes(self, nodes, roots):
        """Build-defined: an SDF expression forest (operators of util/primitive_operations/ over
        sphere / box / torus / mandelbulb leaves); see Context.scene_from_nodes."""
        self.ctx.scene_from_nodes(nodes, roots, self.accel_enum)
        self._uploaded = True
        self._session = None

    # ---- object CRUD on sphere scenes (the reference README's third plan; rm_scene_edit_spheres) ----
    def editSpheres(self, edits):
        """Applies a batch of edits to this scene's sphere list in place: edits = [("set", i, centre, radius),
        ("insert", i, centre, radius), ("remove", i), ...], indices in object order (what objectAt returns) at the moment
        each edit applies.  The scene must be a sphere list (loadSpheres, or preset 0..4); it is the uploaded scene
        afterwards, exactly as loadSpheres(edited list) would leave it.  All or nothing.  With a mesh session open
        (meshSession) the edit goes through it, so its tiles follow the scene."""
        edits = list(edits)
        self._activate()
        if self._session is not None:
            self._session.edit_spheres(edits)
        else:
            self.ctx.edit_spheres(edits)
        if edits:
            self._uploaded = True

    def setSphere(self, i, centre, radius):
        self.editSpheres([("set", i, centre, radius)])

    def insertSphere(self, i, centre, radius):
        self.editSpheres([("insert", i, centre, radius)])

    def removeSphere(self, i):
        self.editSpheres([("remove", i)])

    def updateTime(self, time):  # scene.ts:135-140
        self.ctx.scene_set_time(time)
        self.time = float(time)

    @property
    def preset_for_job(self):
        return N.RM_SCENE_UPLOADED if self._uploaded else self.currentPresetIndex

    def getDistance(self, position, sdfEvaluationCounter=None):  # scene.ts:144-190
        self._activate()
        d, c = self.ctx.scene_distance(np.asarray(position, np.float32).reshape(1, 3))
        if sdfEvaluationCounter is not None:
            sdfEvaluationCounter["count"] += int(c[0])
        return float(d[0])

    def getDistances(self, points):
        self._activate()
        return self.ctx.scene_distance(points)

    def distanceField(self, origin, du, dv, dw=None, shape=(1, 1), dist32=False, count=True, device=False, exact=False):
        """getDistance at every point origin + i * du + j * dv + k * dw of a lattice formed on the device, at this scene's
        own time (Context.field) -> (dist, count) shaped [nw, nv, nu], [nv, nu] for shape = (nu, nv).  exact=True: the exact
        field -- min over ALL objects -- whatever acceleration structure the scene has (option `exact` for this call)."""
        self._activate()
        return self.ctx.field(origin, du, dv, dw, shape=shape, time=self.time, dist32=dist32, count=count, device=device, exact=exact)

    def getNormal(self, position, exact=False):
        """Raymarcher.getNormal (raymarcher.ts:123-135) at a point, at this scene's own time (Context.points): three floats.
        exact=True: the gradient of the exact field."""
        self._activate()
        r = self.ctx.points(np.asarray(position, np.float32).reshape(1, 3), object=False, time=self.time, exact=exact)
        return [float(x) for x in r.normal[0]]

    def nearestObject(self, position, exact=False):
        """Index of the object that attains getDistance at a point (a 3D cursor), at this scene's own time; -1: none.
        exact=True: among ALL objects (under a BVH or an octree getDistance only sees the leaves at the point)."""
        self._activate()
        return int(self.ctx.points(np.asarray(position, np.float32).reshape(1, 3), normal=False, time=self.time, exact=exact).object[0])

    def projectToSurface(self, points, steps=4, tol=1e-4, exact=False):
        """`points` dropped onto the surface getDistance = 0 at this scene's own time (Context.project) -> (position, dist,
        steps).  An empty octree leaf has no gradient and a BVH's distance over-estimates: exact=True projects along the exact field."""
        self._activate()
        return self.ctx.project(points, steps=steps, tol=tol, time=self.time, exact=exact)

    def toMesh(self, origin=None, du=None, dv=None, dw=None, shape=None, iso=0.0, cells=(64, 64, 64), margin=None, device=False,
               triangles=False, attributes=False, snap=0, tol=1e-4, sparse=False, lipschitz=1.0, exact=False, sharp=False, refine=2,
               rank_tol=0.1, reach=1.0):
        """The surface getDistance = iso at this scene's own time as (vertices float32 [V, 3], quads uint32 [Q, 4]) -- or
        triangles uint32 [2Q, 3] --, extracted on the device (Context.mesh): over the lattice origin + i * du + j * dv + k * dw
        of `shape` points, or, without one, over the root box in `cells` cells (Context.mesh_box).  attributes=True adds
        (normals, objects) per vertex, the vertices snapped onto the surface by up to `snap` steps (Context.mesh_field).
        sparse=True samples and meshes only the 8 x 8 x 8-cell blocks that can hold the surface when the exact field is
        `lipschitz`-Lipschitz (Context.mesh_sparse, order "dense"): the same mesh, and lattices the dense path cannot hold.
        exact=True meshes the exact field (offset surfaces, octree scenes), attributes included.  sharp=True keeps edges and
        corners: the vertices are dual contouring's (Context.sharpen with refine, rank_tol and reach), the faces the same."""
        self._activate()
        more = dict(iso=iso, time=self.time, device=device, triangles=triangles, attributes=attributes, snap=snap, tol=tol, exact=exact, sharp=sharp,
                    refine=refine, rank_tol=rank_tol, reach=reach)
        if origin is None:
            return self.ctx.mesh_box(cells, margin=margin, sparse=sparse, lipschitz=lipschitz, **more)
        if sparse:
            return self.ctx.mesh_sparse(origin, du, dv, dw, shape, lipschitz=lipschitz, **more)
        return self.ctx.mesh(origin, du, dv, dw, shape, **more)

    def measure(self, origin=None, du=None, dv=None, dw=None, shape=None, iso=0.0, cells=(64, 64, 64), margin=None, lipschitz=1.0, sparse=True,
                exact=True):
        """How much there is of the solid getDistance < iso at this scene's own time -> a Measure (Context.measure): the
        integer record (n_inside, sum1, sum2, crossings, the index box, ...), `.world` (volume, centroid, second moments,
        projected areas, an area estimate) and `.inertia()`.  Over the lattice origin + i * du + j * dv + k * dw of `shape`
        points, or, without one, over the root box in `cells` cells (Context.measure_box).  sparse, lipschitz, exact: as
        Context.measure."""
        self._activate()
        more = dict(iso=iso, time=self.time, lipschitz=lipschitz, sparse=sparse, exact=exact)
        if origin is None:
            return self.ctx.measure_box(cells, margin=margin, **more)
        return self.ctx.measure(origin, du, dv, dw, shape, **more)

    def parts(self, origin=None, du=None, dv=None, dw=None, shape=None, iso=0.0, cells=(64, 64, 64), margin=None, side="inside", records=64,
              device=False, exact=True):
        """The connected pieces of the solid getDistance < iso (side="outside": of what surrounds it) at this scene's own
        time -> Parts (Context.parts): `.labels`, `.n_parts`, `.n_set`, `.measures` (a Measure per part), `.by_size()`,
        `.touches_border(p)`, `.select(values, keep)`.  Over the lattice origin + i * du + j * dv + k * dw of `shape` points,
        or, without one, over the root box in `cells` cells (Context.parts_box)."""
        self._activate()
        more = dict(iso=iso, time=self.time, side=side, records=records, device=device, exact=exact)
        if origin is None:
            return self.ctx.parts_box(cells, margin=margin, **more)
        return self.ctx.parts(origin, du, dv, dw, shape, **more)

    def edt(self, origin=None, du=None, dv=None, dw=None, shape=None, iso=0.0, cells=(64, 64, 64), margin=None, side="inside", device=False,
            exact=True):
        """How far inside the solid getDistance < iso (side="outside": outside it) every lattice point lies, at this scene's
        own time -> Edt (Context.edt): `.d2` (squared index distances, exact), `.max_d2`, `.at`, `.inradius`, `.distance()`,
        `.eroded(r2)`, `.max_by_part(parts)`.  Over the lattice origin + i * du + j * dv + k * dw of `shape` points, or,
        without one, over the root box in `cells` cells (Context.edt_box)."""
        self._activate()
        more = dict(iso=iso, time=self.time, side=side, device=device, exact=exact)
        if origin is None:
            return self.ctx.edt_box(cells, margin=margin, **more)
        return self.ctx.edt(origin, du, dv, dw, shape, **more)

    def meshSession(self, origin, du, dv, dw, shape, iso=0.0, lipschitz=1.0):
        """Opens a mesh session on this scene at its own time (Context.mesh_session) and returns it: session.mesh() is
        toMesh(sparse=True, exact=True) over the lattice, and from now on editSpheres / setSphere / insertSphere /
        removeSphere re-sample only the tiles the edit can reach.  Loading another scene closes the session."""
        self._activate()
        self._session = self.ctx.mesh_session(origin, du, dv, dw, shape, iso=iso, time=self.time, lipschitz=lipschitz)
        return self._session

    def info(self):
        self._activate()
        return self.ctx.scene_info()

    def getObject(self, i):
        """Scene.objectSDFs[i] as an expression tree (rm_scene_object): [(type, child_a, child_b, world_to_local, params)],
        operands first, the object's root last -- what loadNodes takes back (as nodes, roots=[len(nodes) - 1])."""
        self._activate()
        return self.ctx.scene_object(i)

    def objectAt(self, x, y, width, height, algorithm="sphere-tracer"):
        """Index of the object under pixel (x, y) of a width x height frame from this scene's camera at its time
        (runRaymarcher's ray for that pixel, raymarcher.ts:73,83-88, picked with `algorithm`); -1 when the ray hits nothing."""
        if not (0 <= int(x) < int(width) and 0 <= int(y) < int(height)):
            raise ValueError("pixel (%d, %d) is outside the %d x %d frame" % (x, y, width, height))
        self._activate()
        org, dirs = camera_rays(int(width), int(height), self.camera.pitch, self.camera.yaw, int(y), int(y) + 1)
        d = dirs[int(x):int(x) + 1]
        return int(self.ctx.pick(org.reshape(1, 3), d, algorithm, normal=False, time=self.time)[4][0])

    def _activate(self):
        if self._uploaded:
            return  # rm_scene_from_spheres already made it active
        self.ctx.scene_from_preset(self.currentPresetIndex, self.accel_enum)


def _job(scene, width, height, time, yStart, yEnd, algorithm, overshootFactor=None, stepSize=None):
    j = N.rm_job()
    j.width, j.height, j.time = int(width), int(height), float(time)
    j.y_start, j.y_end = int(yStart), int(yEnd)
    j.camera_pitch, j.camera_yaw = float(scene.camera.pitch), float(scene.camera.yaw)
    j.algorithm = N.lib().rm_algorithm_from_string(str(algorithm).encode())
    j.scene_preset_index = scene.preset_for_job
    j.acceleration_structure = scene.accel_enum
    # None mirrors JS `undefined` (constructor defaults 1.2 / 0.1); the ABI encodes it as NaN
    j.overshoot_factor = float(overshootFactor) if overshootFactor is not None else float("nan")
    j.step_size = float(stepSize) if stepSize is not None else float("nan")
    return j


class Raymarcher:
    """cpu_algorithms/raymarcher.ts:19-57 (abstract); subclasses name the algorithm."""
    algorithm = "sphere-tracer"

    def getMaxDistance(self):
        return 10

    def runRaymarcher(self, scene, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer,
                      width, height, time=0.0, yStart=0, yEnd=None, shadedBuffer=None, shader="normal", diagnostics=None):
        """raymarcher.ts:46-57.  shadedBuffer/shader are an extension: fused ShadingModel.shade; so is `diagnostics`
        (device buffers only): a CUDA tensor of 32 bytes that receives the sums / max / min of main.ts:528-548 over the
        rendered rows from the render kernel itself (rm_render_attach_diagnostics; read with Context.decode_acc)."""
        if yEnd is None:
            yEnd = height
        job = _job(scene, width, height, time, yStart, yEnd, self.algorithm,
                   getattr(self, "overshootFactor", None), getattr(self, "stepSize", None))
        sh = N.lib().rm_shader_from_string(str(shader).encode())
        scene.ctx.render_tile(job, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer,
                              rgba=shadedBuffer, shader=sh, diag=diagnostics)
        scene.time = float(time)  # raymarcher.ts:58-59 scene.updateTime(time)

    def _ray_march(self, scene, origins, directions, normal):
        scene._activate()
        return scene.ctx.ray_march(origins, directions, self.algorithm, normal=normal, time=scene.time,
                                   overshoot=getattr(self, "overshootFactor", None), step=getattr(self, "stepSize", None))

    def rayMarch(self, scene, rayOrigin, direction, idx, SDFevaluationBuffer, iterationsBuffer):
        """raymarcher.ts:26-33 (the subclass's marcher) for one ray of any origin and direction (rm_ray_march): returns
        the distance travelled and adds its Scene.getDistance and iteration counts at idx, wrapped as Uint16Array += wraps."""
        t, it, sdf, _ = self._ray_march(scene, np.asarray(rayOrigin, np.float32).reshape(1, 3),
                                        np.asarray(direction, np.float32).reshape(1, 3), False)
        SDFevaluationBuffer[idx] = (int(SDFevaluationBuffer[idx]) + int(sdf[0])) & 0xFFFF
        iterationsBuffer[idx] = (int(iterationsBuffer[idx]) + int(it[0])) & 0xFFFF
        return float(t[0])

    def getNormal(self, scene, position, idx, SDFevaluationBuffer):
        """raymarcher.ts:123-135 from four Scene.getDistance evaluations (rm_scene_distance): the offsets stored to
        Float32Arrays, the differences to the Float32Array n, vec3.normalize.  Adds the four counts at idx."""
        scene._activate()
        scene.ctx.scene_set_time(scene.time)
        p = np.asarray(position, np.float32).reshape(3)
        pts = np.repeat(p[None, :], 4, axis=0)
        for a in range(3):  # vec3.fromValues(position[a] - 0.01, ...)
            pts[a + 1, a] = np.float32(np.float64(p[a]) - 0.01)
        dist, cnt = scene.ctx.scene_distance(pts)
        SDFevaluationBuffer[idx] = (int(SDFevaluationBuffer[idx]) + int(cnt.sum())) & 0xFFFF
        n = np.float32(dist[0] - dist[1:4])
        ln = float(np.float64(n[0]) * n[0] + np.float64(n[1]) * n[1] + np.float64(n[2]) * n[2])
        if ln > 0:
            ln = 1 / math.sqrt(ln)
        return np.array([np.float32(np.float64(v) * ln) for v in n], np.float32)

    def rayMarchBatch(self, scene, origins, directions, normal=True):
        """rayMarch (+ getNormal at hits) for a batch of rays in one call: Context.ray_march with this marcher, its
        options and the scene's time -> (t, iters, sdf_calls, normal)."""
        return self._ray_march(scene, origins, directions, normal)

    def pickBatch(self, scene, origins, directions, normal=True):
        """rayMarchBatch plus the object each ray hit (Context.pick with this marcher, its options and the scene's time)
        -> (t, iters, sdf_calls, normal, object)."""
        scene._activate()
        return scene.ctx.pick(origins, directions, self.algorithm, normal=normal, time=scene.time,
                              overshoot=getattr(self, "overshootFactor", None), step=getattr(self, "stepSize", None))

    def lightBatch(self, scene, origins, directions, light_dir=None, bias=0.02, ao_samples=5, ao_step=0.05, ao_strength=1.0):
        """rayMarchBatch with normals plus a shadow term and an ambient-occlusion term at each hit (Context.light with this
        marcher, its options and the scene's time) -> (t, iters, sdf_calls, normal, lit, ao, iters2, sdf_calls2)."""
        scene._activate()
        return scene.ctx.light(origins, directions, light_dir=light_dir, bias=bias, ao_samples=ao_samples, ao_step=ao_step,
                               ao_strength=ao_strength, algorithm=self.algorithm, time=scene.time,
                               overshoot=getattr(self, "overshootFactor", None), step=getattr(self, "stepSize", None))

    def walkBatch(self, scene, origins, directions, trace=False, cap=200):
        """How this marcher walks each ray (Context.walk with this marcher, its options and the scene's time) -> walks, or
        (walks, steps) with `trace`."""
        scene._activate()
        return scene.ctx.walk(origins, directions, algorithm=self.algorithm, time=scene.time,
                              overshoot=getattr(self, "overshootFactor", None), step=getattr(self, "stepSize", None), trace=trace, cap=cap)


class SphereTracer(Raymarcher):  # cpu_algorithms/sphereTracer.ts
    algorithm = "sphere-tracer"


class FixedStep(Raymarcher):  # cpu_algorithms/fixedStep.ts
    algorithm = "fixed-step"

    def __init__(self, stepSize=None):
        self.stepSize = stepSize


class AdaptiveStep(Raymarcher):  # cpu_algorithms/adaptiveStep.ts
    algorithm = "adaptive-step"


class AdaptiveStepV2(Raymarcher):
    algorithm = "adaptive-step-v2"

    def __init__(self, overshootFactor=None):
        self.overshootFactor = overshootFactor


class AdaptiveStepV3(AdaptiveStepV2):
    algorithm = "adaptive-step-v3"


def createRaymarcher(algorithm, overshootFactor=None, stepSize=None):
    """raymarchWorker.ts:49-68 (unknown -> SphereTracer)."""
    if algorithm == "fixed-step":
        return FixedStep(stepSize)
    if algorithm == "adaptive-step":
        return AdaptiveStep()
    if algorithm == "adaptive-step-v2":
        return AdaptiveStepV2(overshootFactor)
    if algorithm == "adaptive-step-v3":
        return AdaptiveStepV3(overshootFactor)
    return SphereTracer()


class ShadingModel:
    """util/shading_models/shadingModel.ts:8-17."""
    name = "normal"

    def __init__(self, ctx: Optional[Context] = None, device=0):
        self._ctx = ctx
        self._device = device

    def shade(self, shadedBuffer, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer, width, height):
        if self._ctx is None:
            self._ctx = Context(self._device)
        sh = N.lib().rm_shader_from_string(self.name.encode())
        self._ctx.shade(sh, width, height, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer,
                        shadedBuffer)
        return shadedBuffer


class NormalModel(ShadingModel):
    name = "normal"


class PhongModel(ShadingModel):
    name = "phong"


class SDFHeatmap(ShadingModel):
    name = "sdf-heatmap"


class IterationHeatmap(ShadingModel):
    name = "iteration-heatmap"


class _RangedHeatmap(ShadingModel):
    """Build-defined, beside the factory (createShadingModelFromValue keeps the reference's mapping): the heatmap of one
    counter scaled from 0 to the hi_permille percentile of the frame's own histogram of that counter (Context.counter_hist,
    then Context.shade_ranged from the same record, with no host round trip in between on device buffers), so it never wraps
    as counter * 5 % 256 does.  `mask`, `bin_shift`: as counter_hist takes them.  After shade(), `hist` holds the frame's
    record buffer (Context.decode_hists)."""
    counter = "sdf"

    def __init__(self, ctx: Optional[Context] = None, device=0, hi_permille=1000, mask="all", bin_shift=0):
        super().__init__(ctx, device)
        self.hi_permille, self.mask, self.bin_shift = int(hi_permille), mask, int(bin_shift)
        self.hist = None

    def shade(self, shadedBuffer, depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer, width, height):
        if self._ctx is None:
            self._ctx = Context(self._device)
        values = SDFevaluationBuffer if self.counter == "sdf" else iterationsBuffer
        masked = self.mask not in ("all", 0)
        self.hist = self._ctx.counter_hist(values if self.counter == "sdf" else None, values if self.counter == "iters" else None,
                                           normal=normalBuffer if masked else None, mask=self.mask, bin_shift=self.bin_shift,
                                           percentiles=(0, self.hi_permille), width=width, rows=height, n_frames=1)
        self._ctx.shade_ranged(self.counter, values, shadedBuffer, hist=self.hist, width=width, rows=height, n_frames=1)
        return shadedBuffer


class RangedSDFHeatmap(_RangedHeatmap):
    name = "ranged-sdf-heatmap"
    counter = "sdf"


class RangedIterationHeatmap(_RangedHeatmap):
    name = "ranged-iteration-heatmap"
    counter = "iters"


def createShadingModelFromValue(selectedModel, ctx=None):  # main.ts:33-45
    return {"phong": PhongModel, "sdf-heatmap": SDFHeatmap,
            "iteration-heatmap": IterationHeatmap}.get(selectedModel, NormalModel)(ctx)


@dataclass
class Job:  # raymarchWorker.ts:10-22
    width: int
    height: int
    time: float = 0.0
    yStart: int = 0
    yEnd: int = 0
    camera: dict = field(default_factory=lambda: {"pitch": 0.0, "yaw": 0.0})
    algorithm: str = "sphere-tracer"
    scenePresetIndex: int = 0
    accelerationStructure: str = "None"
    overshootFactor: Optional[float] = None
    stepSize: Optional[float] = None


@dataclass
class Result:  # raymarchWorker.ts:24-31
    yStart: int
    yEnd: int
    depth: np.ndarray
    normal: np.ndarray
    sdfEval: np.ndarray
    iters: np.ndarray


class RaymarchWorker:
    """workers/raymarchWorker.ts: stateless between jobs as far as results go; the scene the
    job names stays resident in HBM between jobs."""

    def __init__(self, ctx: Optional[Context] = None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self._scene = None

    def onmessage(self, job: Job) -> Result:  # raymarchWorker.ts:33-92
        if self._scene is None or self._scene.accelerationStructure != job.accelerationStructure:
            self._scene = Scene(job.accelerationStructure, ctx=self.ctx)
        scene = self._scene
        scene.loadPreset(job.scenePresetIndex)
        scene.camera.setAngles(job.camera["pitch"], job.camera["yaw"])
        tileHeight = max(0, job.yEnd - job.yStart)
        depth = np.zeros(job.width * tileHeight, np.uint8)
        normal = np.zeros(job.width * tileHeight * 3, np.uint8)
        sdfEval = np.zeros(job.width * tileHeight, np.uint16)
        iters = np.zeros(job.width * tileHeight, np.uint16)
        alg = createRaymarcher(job.algorithm, job.overshootFactor, job.stepSize)
        alg.runRaymarcher(scene, depth, normal, sdfEval, iters, job.width, job.height, job.time, job.yStart, job.yEnd)
        return Result(job.yStart, job.yEnd, depth, normal, sdfEval, iters)


def renderFrame(workers, width, height, scenePresetIndex, accelerationStructure, pitch=0.0, yaw=0.0,
                algorithm="sphere-tracer", time=0.0):
    """main.ts:444-468: partition rows over the workers, gather tiles into frame buffers."""
    n = len(workers)
    depthBuffer = np.zeros(width * height, np.uint8)
    normalBuffer = np.zeros(width * height * 3, np.uint8)
    SDFevaluationBuffer = np.zeros(width * height, np.uint16)
    iterationsBuffer = np.zeros(width * height, np.uint16)
    for i, w in enumerate(workers):
        yStart, yEnd = partition_rows(height, n, i)
        if yStart >= yEnd:
            continue
        r = w.onmessage(Job(width, height, time, yStart, yEnd, {"pitch": pitch, "yaw": yaw}, algorithm,
                            scenePresetIndex, accelerationStructure))
        pixelOffset = r.yStart * width
        depthBuffer[pixelOffset:pixelOffset + r.depth.size] = r.depth
        SDFevaluationBuffer[pixelOffset:pixelOffset + r.sdfEval.size] = r.sdfEval
        iterationsBuffer[pixelOffset:pixelOffset + r.iters.size] = r.iters
        normalBuffer[pixelOffset * 3:pixelOffset * 3 + r.normal.size] = r.normal
    return depthBuffer, normalBuffer, SDFevaluationBuffer, iterationsBuffer


def diagnostics(ctx, SDFevaluationBuffer, iterationsBuffer):
    """main.ts:528-548 on the device: averages as the page shows them."""
    d = ctx.reduce_counters(SDFevaluationBuffer, iterationsBuffer)
    n = max(1, d["total_pixels"])
    d["average_sdf_calls"] = d["total_sdf"] / n
    d["average_iterations"] = d["total_iters"] / n
    return d


def save_obj(path, vertices, faces, normals=None, objects=None):
    """Writes a mesh as Wavefront OBJ text: one `v x y z` line per vertex (repr of the float32 value: it reads back exactly),
    one `f a b c [d]` line per face with 1-based indices.  With `normals` (float32 [V, 3], one per vertex: what the meshers
    return with attributes=True) a `vn x y z` line per vertex follows the vertices and the faces read `f a//a b//b ...`.  With
    `objects` (int32 [V]) the faces are sorted, stably, by the object of their first vertex and each run stands under a
    `g object_<k>` line (`g background` for -1).  No materials.  With neither: the plain file."""
    host = lambda a: np.asarray(a.cpu() if _is_torch(a) else a)  # noqa: E731
    v = host(vertices).astype(np.float32, copy=False).reshape(-1, 3)
    f = host(faces)
    f = (f.view(np.uint32) if f.dtype == np.int32 else f).astype(np.int64).reshape(len(f), -1) + 1
    corner = (lambda i: "%d//%d" % (i, i)) if normals is not None else str
    lines = ["f " + " ".join(corner(int(i)) for i in row) + "\n" for row in f]
    vn = None if normals is None else host(normals).astype(np.float32, copy=False).reshape(-1, 3)
    obj = None if objects is None else host(objects).astype(np.int64).reshape(-1)
    if (vn is not None and len(vn) != len(v)) or (obj is not None and len(obj) != len(v)):
        raise ValueError("normals and objects must hold one entry per vertex")
    with open(path, "w") as out:
        out.write("".join("v %r %r %r\n" % tuple(float(x) for x in row) for row in v))
        if vn is not None:
            out.write("".join("vn %r %r %r\n" % tuple(float(x) for x in row) for row in vn))
        if obj is None:
            out.write("".join(lines))
            return
        of_face = obj[f[:, 0] - 1] if len(f) else np.zeros(0, np.int64)
        last = None
        for k in np.argsort(of_face, kind="stable"):
            if last is None or of_face[k] != last:
                last = of_face[k]
                out.write("g background\n" if last < 0 else "g object_%d\n" % last)
            out.write(lines[k])
