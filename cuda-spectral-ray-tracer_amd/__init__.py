"""MI355X-native spectral path tracer: hot-path replacement for PieSil/CUDA-spectral-ray-tracer.

The product is libsrt_hip.so (hand-written gfx950 kernels behind the C-ABI of include/srt_c_api.h).  This
package is the Python face of that ABI (ctypes) plus the torch.distributed plumbing of the multi-GPU gather.
Importing it never computes anything and never falls back to a CPU implementation.
"""
from . import binding
from .binding import (BVH_REFERENCE, BVH_SAH, SCENE_CORNELL, SCENE_MESH100K, SCENE_PRISM, SCENE_RANDOM_SPHERES,
                      SCENE_TRIS, CameraData, Material, SrtError, TriIn)
from .scene import Scene, camera_init
from .renderer import (Comm, Renderer, ray_batch, direct_light_config, render_direct, light_stats, meter_config, tone_config, meter_decide, render_exposed, present_config, render_presented, despeckle_config, render_despeckled, temporal_config, temporal_vg_config, temporal_stats, motion_stats, render_interactive, render_interactive_multi, gather_parts, GATHER_PARTS, render_animated, denoise_config, denoise_vg_config, render_denoised, render_adaptive_denoised, render_developed_denoised, render_adaptive_spectral, feature_means, film_to_xyz, pixels_per_lane, profile_child_order, reference_grid, render_adaptive, render_image,
                       render_developed, render_features, render_progressive, render_spectral, sensor_response, render_streams, spectral_radiance, spectral_wavelengths, tree_tuning, tune_tree_for_throughput)
from . import tiles

__all__ = ["binding", "Scene", "camera_init", "Renderer", "ray_batch", "direct_light_config", "render_direct", "light_stats", "Comm", "reference_grid", "render_image", "render_progressive", "render_adaptive", "render_spectral", "render_developed", "sensor_response", "render_streams", "render_features", "feature_means", "meter_config", "tone_config", "meter_decide", "render_exposed", "present_config", "render_presented", "despeckle_config", "render_despeckled", "temporal_config", "temporal_vg_config", "temporal_stats", "motion_stats", "render_interactive", "render_interactive_multi", "gather_parts", "GATHER_PARTS", "render_animated", "denoise_config", "denoise_vg_config", "render_denoised", "render_adaptive_denoised", "render_developed_denoised", "render_adaptive_spectral",
           "spectral_wavelengths", "spectral_radiance", "film_to_xyz", "profile_child_order", "tune_tree_for_throughput", "tree_tuning", "pixels_per_lane", "tiles", "SrtError",
           "TriIn", "Material", "CameraData", "BVH_REFERENCE", "BVH_SAH", "SCENE_CORNELL", "SCENE_PRISM",
           "SCENE_TRIS", "SCENE_RANDOM_SPHERES", "SCENE_MESH100K"]
