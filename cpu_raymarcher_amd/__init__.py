"""cpu_raymarcher_amd -- MI355X-native drop-in for the per-pixel sphere-tracing render path of
vxlerian/cpu-raymarcher (hand-written HIP for gfx950 behind the C ABI of include/rm_raymarch.h).

Importing this package loads cpu_raymarcher_amd/librm_hip.so and fails loudly if it is not
built: there is no CPU fallback on the product path.
"""
from . import _native
from ._native import RmError, RmUnsupported, RM_SCENE_UPLOADED
from ._native import STEP_DTYPE, WALK_DTYPE, WALK_ENDS  # the records Context.walk returns

_native.lib()  # raise now, not at first render, when the HIP library is missing

from .context import (Context, Edt, Measure, MeasureWorld, MeshSession, camera_from_angles, camera_rays, lattice_cubic, make_lattice,  # noqa: E402
                      make_transform, measure_world, Parts, partition_rows, percentile, phong_light, scale_transform, slice_lattice, sweep_views)
from .host import (ALGORITHMS, SHADERS, AdaptiveStep, AdaptiveStepV2, AdaptiveStepV3, Camera, FixedStep,  # noqa: E402
                   IterationHeatmap, Job, NormalModel, PhongModel, RangedIterationHeatmap, RangedSDFHeatmap, Raymarcher,
                   RaymarchWorker, Result, Scene,
                   SDFHeatmap, ShadingModel, SphereTracer, createRaymarcher, createShadingModelFromValue,
                   diagnostics, renderFrame, save_obj)

__all__ = [n for n in dir() if not n.startswith("_")]
