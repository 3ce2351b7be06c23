"""optix-test-smallpt_amd: MI355X-native replacement for the radiance()/intersect() hot path of
Celeborn2BeAlive/optix-test-smallpt.  The compute path is the gfx950 megakernel behind the C-ABI of
include/smallpt_mi355x.h (csrc/); this package is the thin host-side mirror of the reference's
scene structs and render entry points.  Import name: ``optix_test_smallpt_amd`` (see the shim at
the repository root)."""
from ._lib import (INTERNAL_SYMBOLS, LIB_PATH, MULTI_SYMBOLS, SYMBOLS, SptCamera, SptDemodParams, SptDenoiseParams, SptDenoiseVarParams, SptDisplayParams, SptInstance, SptTemporalParams, SptTemporalVarParams, SptMaterial, SptMesh, SptMultiStats, SptPath, SptSphere, SptStats,  # noqa: F401
                   load_library, load_multi_library)
from .renderer import (ACCEL_AUTO, AOV_KINDS, AOV_SET_KINDS, ACCEL_BVH, ACCEL_BVH_FAST, ACCEL_EXHAUSTIVE, ACCEL_GRID, AOV_EMISSION, DemodParams, DenoiseParams, DenoiseVarParams, DisplayParams, TemporalParams, TemporalVarParams, temporal_history_bytes, camera_inverse, DISPLAY_FLIP_Y, DISPLAY_RGB8, DISPLAY_RGBA8, DISPLAY_SRC_ACCUM, DISPLAY_SRC_DENOISED, DISPLAY_SRC_DENOISED_VAR, FLAG_NORMALISE, MultiRenderer, ProgressiveRenderer, Renderer, SptError, pinhole_camera,  # noqa: F401
                       smallpt_camera, to_int, write_ppm, environment_radiance, display_thresholds, display_quantise_host, write_ppm_rgb8)
from .scene import (DIFF, HIT_DTYPE, environment_from_json, INSTANCE_DTYPE, PATH_DTYPE, RAY_DTYPE, RAY_RANGE_DTYPE, REFR, SPEC, SPHERE_DTYPE, TriMesh, cornell9, make_sphere_trimesh,  # noqa: F401
                    make_spheres, meshes_from_json, meshes_to_json, random_spheres, single_triangle_scene, spheres_from_json,
                    spheres_to_json)

__all__ = ["Renderer", "DemodParams", "DenoiseParams", "DenoiseVarParams", "DisplayParams", "TemporalParams", "TemporalVarParams", "temporal_history_bytes", "camera_inverse", "display_thresholds", "display_quantise_host", "write_ppm_rgb8", "MultiRenderer", "ProgressiveRenderer", "SptError", "smallpt_camera", "pinhole_camera", "cornell9", "random_spheres", "make_spheres",
           "spheres_from_json", "spheres_to_json", "SPHERE_DTYPE", "DIFF", "SPEC", "REFR",
           "load_library", "to_int", "write_ppm", "FLAG_NORMALISE", "ACCEL_EXHAUSTIVE", "ACCEL_BVH", "ACCEL_BVH_FAST", "ACCEL_AUTO", "ACCEL_GRID"]
