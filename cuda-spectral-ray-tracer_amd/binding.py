"""ctypes binding of the C-ABI declared in include/srt_c_api.h (libsrt_hip.so).

Nothing in here computes: it declares the structs / prototypes and turns negative status codes into
exceptions.  There is no fallback path: if the shared library is missing, loading raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRT_LIB_PATH") or os.path.join(_HERE, "libsrt_hip.so")   # (override: kernel experiments only)

N_CIE = 95
TILE_PLANES = 9
TILE_LANES = 64

SCENE_CORNELL, SCENE_PRISM, SCENE_TRIS, SCENE_RANDOM_SPHERES, SCENE_MESH100K = 0, 1, 2, 100, 101
BVH_REFERENCE, BVH_SAH = 0, 1
MAT_LAMBERTIAN, MAT_METALLIC, MAT_DIELECTRIC, MAT_EMISSIVE, MAT_NO_MAT = 0, 1, 2, 4, 6


class TriIn(C.Structure):
    _fields_ = [("v0", C.c_float * 3), ("v1", C.c_float * 3), ("v2", C.c_float * 3),
                ("mat_index", C.c_uint32), ("aa_plane", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("col", C.c_float * 3), ("reflection_fuzz", C.c_float), ("material_type", C.c_uint32),
                ("spectral_distribution", C.c_float * N_CIE), ("emission_power", C.c_float),
                ("sellmeier_B", C.c_float * 3), ("sellmeier_C", C.c_float * 3)]


class CameraData(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32),
                ("pixel_delta_u", C.c_float * 3), ("pixel_delta_v", C.c_float * 3), ("pixel00_loc", C.c_float * 3),
                ("defocus_angle", C.c_float),
                ("camera_center", C.c_float * 3), ("defocus_disk_u", C.c_float * 3), ("defocus_disk_v", C.c_float * 3)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("paths", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64),
                ("box_tests", C.c_uint64), ("util", C.c_uint64 * 9), ("reserved", C.c_uint64 * 2), ("shade", C.c_uint64 * 4),
                ("waves", C.c_uint64 * 4), ("hits", C.c_uint64)]


class Calibration(C.Structure):
    _fields_ = [("wave_cycles_mean", C.c_double), ("wave_cycles_max", C.c_double), ("wall_ms", C.c_double),
                ("instr_per_wave", C.c_uint64), ("n_waves", C.c_uint32), ("n_cu", C.c_uint32), ("waves_per_simd", C.c_uint32),
                ("reserved", C.c_uint32), ("wave_cycles_min", C.c_double)]


class Adaptive(C.Structure):
    """srt_adaptive: the stopping criterion of an adaptive accumulation (srt_c_api.h)"""
    _fields_ = [("rel_tol", C.c_float), ("abs_tol", C.c_float), ("min_spp", C.c_uint32), ("reserved", C.c_uint32)]


class Denoise(C.Structure):
    """srt_denoise: levels and sigmas of the a-trous denoiser (srt_c_api.h)"""
    _fields_ = [("levels", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float), ("reserved", C.c_uint32 * 3)]


class DenoiseVG(C.Structure):
    """srt_denoise_vg: levels, sigmas and variance floor of the variance-guided a-trous denoiser (srt_c_api.h)"""
    _fields_ = [("levels", C.c_uint32), ("sigma_variance", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float), ("variance_floor", C.c_float), ("reserved", C.c_uint32 * 2)]


class Meter(C.Structure):
    """srt_meter: the metered rectangle (all zero: the whole chunk), the percentile, the key it is anchored at and the gain clamps (srt_c_api.h)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("percentile_ppm", C.c_uint32),
                ("key", C.c_float), ("gain_min", C.c_float), ("gain_max", C.c_float), ("reserved", C.c_uint32 * 4)]


class MeterResult(C.Structure):
    """srt_meter_result: the pixel counts of a metering, the reference bin, its midpoint luminance and the gain decided (srt_c_api.h)"""
    _fields_ = [("metered", C.c_uint64), ("dark", C.c_uint64), ("nonfinite", C.c_uint64), ("bin_ref", C.c_uint32),
                ("y_ref", C.c_float), ("gain", C.c_float), ("reserved", C.c_uint32)]


class Tone(C.Structure):
    """srt_tone: the tone curve (0 linear, 1 extended Reinhard), the exposure gain and the white point (srt_c_api.h)"""
    _fields_ = [("curve", C.c_uint32), ("gain", C.c_float), ("white", C.c_float), ("reserved", C.c_uint32 * 5)]


class ToneResult(C.Structure):
    """srt_tone_result: the pixels the tone kernel counted as blown, crushed and non-finite (srt_c_api.h)"""
    _fields_ = [("blown", C.c_uint64), ("crushed", C.c_uint64), ("nonfinite", C.c_uint64)]


SCENE_IMAGES = {"nodes": 0, "nodes_sw": 1, "fringe": 2, "tris": 3, "shade": 4}      # SRT_IMAGE_* (srt_c_api.h)
GATHER_PARTS = {"sums": 1, "counts": 2, "features": 4, "film": 8}      # SRT_GATHER_* (srt_c_api.h)
PRESENT_SOURCES = {"accum": 0, "denoise": 1, "denoise_vg": 2, "denoise_mv": 3, "develop": 4}      # SRT_PRESENT_* (srt_c_api.h)


class PresentCfg(C.Structure):
    """srt_present_cfg: the source of a presented picture, its exposure (metered or given), its tone curve and the configuration of the
    stage the source runs (srt_c_api.h)"""
    _fields_ = [("source", C.c_uint32), ("metered", C.c_uint32), ("meter", Meter), ("tone", Tone), ("denoise", Denoise), ("denoise_vg", DenoiseVG),
                ("response3", C.POINTER(C.c_float)), ("scale", C.c_float), ("reserved", C.c_uint32 * 5)]


class PresentResult(C.Structure):
    """srt_present_result: the metering (zero when the gain was given) and the tone counters of a presented picture (srt_c_api.h)"""
    _fields_ = [("meter", MeterResult), ("tone", ToneResult)]


class Despeckle(C.Structure):
    """srt_despeckle: window radius, rank (parts per million), gain and floor of the firefly filter (srt_c_api.h)"""
    _fields_ = [("radius", C.c_uint32), ("rank_ppm", C.c_uint32), ("gain", C.c_float), ("floor", C.c_float), ("reserved", C.c_uint32 * 4)]


class DespeckleResult(C.Structure):
    """srt_despeckle_result: the pixels the firefly filter clamped, found non-finite and found without a valid neighbour (srt_c_api.h)"""
    _fields_ = [("clamped", C.c_uint64), ("nonfinite", C.c_uint64), ("alone", C.c_uint64)]


class Temporal(C.Structure):
    """srt_temporal: the blend floor, the history cap and the three rejection thresholds of the temporal reprojection (srt_c_api.h)"""
    _fields_ = [("alpha_min", C.c_float), ("max_len", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float), ("reserved", C.c_uint32 * 3)]


class TemporalResult(C.Structure):
    """srt_temporal_result: the pixels the stage blended, took fresh (of those: off-screen, rejected) and found non-finite, the calls since
    the history began and whether this call discarded a history of another rectangle (srt_c_api.h)"""
    _fields_ = [("blended", C.c_uint64), ("fresh", C.c_uint64), ("offscreen", C.c_uint64), ("rejected", C.c_uint64), ("nonfinite", C.c_uint64),
                ("history_frames", C.c_uint32), ("history_dropped", C.c_uint32)]


class TemporalVG(C.Structure):
    """srt_temporal_vg: the moments length from which the variance measured across frames guides the filter, and whether the stage is the
    moving one (srt_c_api.h)"""
    _fields_ = [("min_len", C.c_uint32), ("moving", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class MotionResult(C.Structure):
    """srt_motion_result: the pixels whose centre ray hit and missed, the hit pixels whose triangle moved, and of those the ones whose
    previous point could not be formed (srt_c_api.h)"""
    _fields_ = [("hit", C.c_uint64), ("miss", C.c_uint64), ("moved", C.c_uint64), ("degenerate", C.c_uint64)]


class TreeTuning(C.Structure):
    """srt_tree_tuning: what srt_tune_tree_for_throughput found and did (srt_c_api.h)"""
    _fields_ = [("pixels_per_lane", C.c_double), ("throughput_bound", C.c_uint32), ("reinsertion", C.c_uint32),
                ("probe_width", C.c_uint32), ("probe_height", C.c_uint32), ("probe_spp", C.c_uint32), ("nodes_swapped", C.c_uint32),
                ("order_status", C.c_int32), ("segments", C.c_uint32)]


class TileScheduleInfo(C.Structure):
    """srt_tile_schedule_info: the scheduler's arguments for the context's pixel queue and what it answered (srt_c_api.h)"""
    _fields_ = [("tiles_local", C.c_uint32), ("n_rows", C.c_uint32), ("cost_max", C.c_uint32), ("n_waves_plan", C.c_uint32),
                ("split_load_pct", C.c_uint32), ("order_max_pct", C.c_uint32), ("streams", C.c_uint32), ("reserved", C.c_uint32)]


class QueryInfo(C.Structure):
    """srt_query_info: the last ray-query launch of a context -- kernel ms, persistent waves, inner records cached in LDS, the variant and
    whether it was the any query (srt_c_api.h)"""
    _fields_ = [("ms", C.c_float), ("waves", C.c_uint32), ("n_cached", C.c_uint32), ("narrow_refs", C.c_uint32), ("all_cached", C.c_uint32),
                ("paired", C.c_uint32), ("any", C.c_uint32), ("reserved", C.c_uint32)]


QUERY_MAX_RAYS = 0x7fffffff      # SRT_QUERY_MAX_RAYS (srt_c_api.h)


class Light(C.Structure):
    """srt_light: samples, first sample index, parts (LIGHT_PARTS bits) and seed of a direct-light call (srt_c_api.h)"""
    _fields_ = [("samples", C.c_uint32), ("first_sample", C.c_uint32), ("parts", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64)]


class LightResult(C.Structure):
    """srt_light_result: the sample counters of a direct-light call and the lights in the table (srt_c_api.h)"""
    _fields_ = [("miss", C.c_uint64), ("emitted", C.c_uint64), ("specular", C.c_uint64), ("shaded", C.c_uint64), ("light_rows", C.c_uint64),
                ("light_unoccluded", C.c_uint64), ("sky_rows", C.c_uint64), ("sky_unoccluded", C.c_uint64), ("lights", C.c_uint32),
                ("reserved", C.c_uint32)]


class LightInfo(C.Structure):
    """srt_light_info: kernel ms of the last direct-light call by kind, its rounds, rows per round and query launches (srt_c_api.h)"""
    _fields_ = [("camera_ms", C.c_float), ("shade_ms", C.c_float), ("gather_ms", C.c_float), ("query_ms", C.c_float), ("rounds", C.c_uint32),
                ("rows_per_round", C.c_uint32), ("query_launches", C.c_uint32), ("reserved", C.c_uint32)]


LIGHT_PARTS = {"emitted": 1, "lights": 2, "sky": 4}      # SRT_LIGHT_* (srt_c_api.h)
LIGHT_MAX_SAMPLES = 65536                                 # SRT_LIGHT_MAX_SAMPLES
assert C.sizeof(Light) == 24 and C.sizeof(LightResult) == 72 and C.sizeof(LightInfo) == 32

assert C.sizeof(QueryInfo) == 32
assert C.sizeof(Denoise) == 32 and C.sizeof(DenoiseVG) == 32
assert C.sizeof(Meter) == 48 and C.sizeof(MeterResult) == 40 and C.sizeof(Tone) == 32 and C.sizeof(ToneResult) == 24
assert C.sizeof(PresentCfg) == 184 and C.sizeof(PresentResult) == 64
assert C.sizeof(Despeckle) == 32 and C.sizeof(DespeckleResult) == 24
assert C.sizeof(Temporal) == 32 and C.sizeof(TemporalResult) == 48 and C.sizeof(MotionResult) == 32 and C.sizeof(TemporalVG) == 16
assert C.sizeof(Adaptive) == 16 and C.sizeof(TreeTuning) == 40 and C.sizeof(TileScheduleInfo) == 32
assert C.sizeof(Material) == 428 and C.sizeof(CameraData) == 84 and C.sizeof(TriIn) == 44

# every symbol include/srt_c_api.h declares: name -> (restype, argtypes)
_vp, _i, _u32, _u64, _f, _sz = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t
_fp = C.POINTER(C.c_float)
PROTOTYPES = {
    "srt_version": (C.c_char_p, []),
    "srt_camera_init": (_i, [_i, _i, _f, _fp, _fp, _fp, _f, _f, C.POINTER(CameraData)]),
    "srt_scene_create": (_vp, []),
    "srt_scene_builtin": (_vp, [_i, _u64]),
    "srt_scene_destroy": (None, [_vp]),
    "srt_scene_default_camera": (_i, [_vp, _i, _i, C.POINTER(CameraData)]),
    "srt_scene_set_triangles": (_i, [_vp, C.POINTER(TriIn), _sz]),
    "srt_scene_set_materials": (_i, [_vp, C.POINTER(Material), _sz]),
    "srt_scene_set_background": (_i, [_vp, _fp]),
    "srt_scene_tri_count": (_sz, [_vp]),
    "srt_scene_material_count": (_sz, [_vp]),
    "srt_scene_get_triangles": (_i, [_vp, C.POINTER(TriIn)]),
    "srt_scene_get_materials": (_i, [_vp, C.POINTER(Material)]),
    "srt_scene_get_background": (_i, [_vp, _fp]),
    "srt_scene_get_tri_records": (_i, [_vp, _fp]),
    "srt_material_bake": (_i, [C.POINTER(Material)]),
    "srt_set_reference_quirks": (_i, [_i]),
    "srt_bake_sigmoid_spectrum": (_i, [_fp, _f, _i, _fp]),
    "srt_fit_sigmoid_coeffs": (_i, [_fp, _fp]),
    "srt_color_tables": (_i, [_fp, _fp]),
    "srt_background_spectrum": (_i, [_fp, _fp]),
    "srt_rotation_matrix": (_i, [_f, _i, _fp]),
    "srt_scene_refit": (_i, [_vp, _fp, _sz]),
    "srt_scene_refit_schedule": (_i, [_vp, C.POINTER(_u32), _sz, C.POINTER(_u32)]),
    "srt_scene_build_bvh": (_i, [_vp, _i, _u64]),
    "srt_scene_order_children": (_i, [_vp, _fp]),
    "srt_scene_optimise_bvh": (_i, [_vp, C.c_int]),
    "srt_scene_optimise_bvh_for_rays": (_i, [_vp, C.c_int, _fp, _sz]),
    "srt_scene_bvh_ray_cost": (_i, [_vp, _fp, _sz, C.POINTER(C.c_double)]),
    "srt_scene_is_paired": (_i, [_vp]),
    "srt_scene_node_count": (_sz, [_vp]),
    "srt_scene_bvh_depth": (_i, [_vp]),
    "srt_scene_get_bvh": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _fp]),
    "srt_create": (_i, [_i, C.POINTER(_vp)]),
    "srt_destroy": (None, [_vp]),
    "srt_last_error": (C.c_char_p, [_vp]),
    "srt_upload_scene": (_i, [_vp, _vp]),
    "srt_refit_vertices": (_i, [_vp, _fp, _sz]),
    "srt_refit_vertices_dev": (_i, [_vp, _vp, _sz]),
    "srt_refit_last_ms": (_i, [_vp, _fp, _fp, C.POINTER(_u32)]),
    "srt_read_scene_image": (_i, [_vp, _i, _vp, _sz, C.POINTER(_sz)]),
    "srt_set_camera": (_i, [_vp, C.POINTER(CameraData)]),
    "srt_launch_plan": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "srt_launch_paired": (_i, [_vp, C.POINTER(_i)]),
    "srt_set_test_knobs": (_i, [_vp, _i, _i, _u32]),
    "srt_get_test_knobs": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_u32), C.POINTER(_i)]),
    "srt_launch_lds_bytes": (_i, [_vp, C.POINTER(_sz)]),
    "srt_init_device_params": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _u64]),
    "srt_set_partition": (_i, [_vp, _u32, _u32]),
    "srt_render_chunk": (_i, [_vp, _u32, _u32, _u32, _u32, _vp]),
    "srt_synchronize": (_i, [_vp]),
    "srt_accum_reset": (_i, [_vp]),
    "srt_render_chunk_accum": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _vp]),
    "srt_accum_samples": (_i, [_vp, C.POINTER(_u32)]),
    "srt_accum_reset_adaptive": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_accum_active": (_i, [_vp, C.POINTER(_u64)]),
    "srt_read_accum_stats": (_i, [_vp, C.POINTER(_u32), _fp, _fp, _u32, _u32]),
    "srt_accum_reset_spectral": (_i, [_vp]),
    "srt_read_spectral": (_i, [_vp, _u32, _u32, _fp, _u32, _u32]),
    "srt_develop_spectral": (_i, [_vp, _fp, _u32, _f, _fp, _u32, _u32]),
    "srt_develop_spectral_srgb": (_i, [_vp, _fp, _f, _fp, _fp, _fp, _u32, _u32]),
    "srt_develop_kat": (_i, [_vp, _fp, _u32, _fp, _u32, _f, _fp]),
    "srt_develop_last_ms": (_i, [_vp, _fp, _fp]),
    "srt_meter_decide": (_i, [C.POINTER(_u32), C.POINTER(Meter), C.POINTER(MeterResult)]),
    "srt_meter_accum": (_i, [_vp, C.POINTER(Meter), C.POINTER(_u32), C.POINTER(MeterResult)]),
    "srt_meter_kat": (_i, [_vp, C.POINTER(Meter), _fp, _u32, _u32, C.POINTER(_u32), C.POINTER(MeterResult)]),
    "srt_expose_accum": (_i, [_vp, C.POINTER(Tone), _fp, _fp, _fp, C.POINTER(ToneResult), _u32, _u32]),
    "srt_expose_kat": (_i, [_vp, C.POINTER(Tone), _fp, _u32, _u32, _fp, _fp, _fp, C.POINTER(ToneResult)]),
    "srt_expose_last_ms": (_i, [_vp, _fp, _fp]),
    "srt_present": (_i, [_vp, C.POINTER(PresentCfg), C.POINTER(C.c_uint8), _sz, _u32, _u32, C.POINTER(PresentResult)]),
    "srt_present_kat": (_i, [_vp, C.POINTER(Tone), _fp, _u32, _u32, C.POINTER(C.c_uint8), C.POINTER(ToneResult)]),
    "srt_present_last_ms": (_i, [_vp, _fp]),
    "srt_despeckle_accum": (_i, [_vp, C.POINTER(Despeckle), _fp, _fp, _fp, _fp, C.POINTER(DespeckleResult), _u32, _u32]),
    "srt_despeckle_kat": (_i, [_vp, C.POINTER(Despeckle), _fp, _u32, _u32, _fp, _fp, C.POINTER(DespeckleResult)]),
    "srt_despeckle_last_ms": (_i, [_vp, _fp]),
    "srt_denoise_features_ds": (_i, [_vp, C.POINTER(Despeckle), C.POINTER(Denoise), _fp, _fp, _fp, _u32, _u32]),
    "srt_present_despeckled": (_i, [_vp, C.POINTER(PresentCfg), C.POINTER(Despeckle), C.POINTER(C.c_uint8), _sz, _u32, _u32, C.POINTER(PresentResult),
                                C.POINTER(DespeckleResult)]),
    "srt_temporal_reset": (_i, [_vp]),
    "srt_temporal_accum": (_i, [_vp, C.POINTER(Temporal), _fp, _fp, _fp, _fp, _fp, C.POINTER(TemporalResult), _u32, _u32]),
    "srt_temporal_kat": (_i, [_vp, C.POINTER(Temporal), C.POINTER(CameraData), C.POINTER(CameraData), _fp, _fp, _fp, _fp, _u32, _u32, _u32, _u32,
                              _fp, _fp, _fp, C.POINTER(TemporalResult)]),
    "srt_denoise_features_temporal": (_i, [_vp, C.POINTER(Temporal), C.POINTER(Despeckle), C.POINTER(Denoise), _fp, _fp, _fp, C.POINTER(TemporalResult),
                                           _u32, _u32]),
    "srt_present_temporal": (_i, [_vp, C.POINTER(PresentCfg), C.POINTER(Temporal), C.POINTER(Despeckle), C.POINTER(C.c_uint8), _sz, _u32, _u32,
                                  C.POINTER(PresentResult), C.POINTER(TemporalResult)]),
    "srt_temporal_last_ms": (_i, [_vp, _fp]),
    "srt_temporal_track_motion": (_i, [_vp, _i]),
    "srt_temporal_tracking": (_i, [_vp, C.POINTER(_i), C.POINTER(_u32)]),
    "srt_surface_motion": (_i, [_vp, _u32, _u32, _u32, _u32, _fp, C.POINTER(C.c_int32), _fp, C.POINTER(MotionResult)]),
    "srt_surface_motion_kat": (_i, [_vp, C.POINTER(CameraData), _fp, _fp, _sz, _u32, _u32, _u32, _u32, _fp, C.POINTER(C.c_int32), _fp,
                                    C.POINTER(MotionResult)]),
    "srt_motion_last_ms": (_i, [_vp, _fp]),
    "srt_temporal_accum_moving": (_i, [_vp, C.POINTER(Temporal), _fp, _fp, _fp, _fp, _fp, C.POINTER(TemporalResult), _u32, _u32, C.POINTER(MotionResult)]),
    "srt_temporal_moving_kat": (_i, [_vp, C.POINTER(Temporal), C.POINTER(CameraData), C.POINTER(CameraData), _fp, _fp, _fp, _fp, _u32, _u32, _u32, _u32,
                                     _fp, _fp, _fp, C.POINTER(TemporalResult), _fp]),
    "srt_denoise_features_temporal_moving": (_i, [_vp, C.POINTER(Temporal), C.POINTER(Despeckle), C.POINTER(Denoise), _fp, _fp, _fp,
                                                  C.POINTER(TemporalResult), _u32, _u32, C.POINTER(MotionResult)]),
    "srt_present_temporal_moving": (_i, [_vp, C.POINTER(PresentCfg), C.POINTER(Temporal), C.POINTER(Despeckle), C.POINTER(C.c_uint8), _sz, _u32, _u32,
                                         C.POINTER(PresentResult), C.POINTER(TemporalResult), C.POINTER(MotionResult)]),
    "srt_denoise_features_temporal_vg": (_i, [_vp, C.POINTER(Temporal), C.POINTER(Despeckle), C.POINTER(DenoiseVG), C.POINTER(TemporalVG), _fp, _fp, _fp, _fp,
                                              C.POINTER(TemporalResult), C.POINTER(_u64), C.POINTER(MotionResult), _u32, _u32]),
    "srt_present_temporal_vg": (_i, [_vp, C.POINTER(PresentCfg), C.POINTER(Temporal), C.POINTER(Despeckle), C.POINTER(TemporalVG), C.POINTER(C.c_uint8), _sz,
                                     _u32, _u32, C.POINTER(PresentResult), C.POINTER(TemporalResult), C.POINTER(_u64), C.POINTER(MotionResult)]),
    "srt_temporal_moments_kat": (_i, [_vp, C.POINTER(Temporal), C.POINTER(CameraData), C.POINTER(CameraData), _fp, _fp, _fp, _fp, _u32, _u32, _u32, _u32,
                                      _fp, _fp, _fp, C.POINTER(TemporalResult), _fp, _fp, _fp]),
    "srt_temporal_variance_kat": (_i, [_vp, _fp, _fp, _fp, _u32, _u32, _u32, _fp, C.POINTER(_u64)]),
    "srt_read_temporal_moments": (_i, [_vp, _fp, _u32, _u32]),
    "srt_temporal_variance_last_ms": (_i, [_vp, _fp]),
    "srt_accum_reset_features": (_i, [_vp]),
    "srt_read_features": (_i, [_vp, _fp, _u32, _u32]),
    "srt_accum_reset_adaptive_features": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_accum_reset_spectral_features": (_i, [_vp]),
    "srt_accum_reset_adaptive_spectral": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_accum_reset_adaptive_spectral_features": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_denoise_developed_counts_kat": (_i, [_vp, C.POINTER(Denoise), _fp, _fp, _fp, _u32, C.POINTER(_u32), _u32, _u32, _fp, _fp]),
    "srt_denoise_developed": (_i, [_vp, C.POINTER(Denoise), _fp, _u32, _f, _fp, _fp, _u32, _u32]),
    "srt_denoise_developed_kat": (_i, [_vp, C.POINTER(Denoise), _fp, _fp, _fp, _u32, _u32, _u32, _u32, _fp, _fp]),
    "srt_denoise_features": (_i, [_vp, C.POINTER(Denoise), _fp, _fp, _fp, _u32, _u32]),
    "srt_denoise_kat": (_i, [_vp, C.POINTER(Denoise), _fp, _fp, _u32, _u32, _u32, _fp]),
    "srt_denoise_last_ms": (_i, [_vp, _fp, _fp, _fp, C.POINTER(_u32)]),
    "srt_denoise_features_vg": (_i, [_vp, C.POINTER(DenoiseVG), _fp, _fp, _fp, _fp, _u32, _u32]),
    "srt_denoise_vg_kat": (_i, [_vp, C.POINTER(DenoiseVG), _fp, _fp, _u32, _u32, _u32, _fp, _fp]),
    "srt_denoise_estimate_last_ms": (_i, [_vp, _fp]),
    "srt_denoise_features_mv": (_i, [_vp, C.POINTER(DenoiseVG), _fp, _fp, _fp, _fp, _u32, _u32]),
    "srt_denoise_mv_kat": (_i, [_vp, C.POINTER(DenoiseVG), _fp, _fp, C.POINTER(_u32), _fp, _u32, _u32, _fp, _fp]),
    "srt_accum_reset_streams": (_i, [_vp, _u32]),
    "srt_accum_streams": (_i, [_vp, C.POINTER(_u32)]),
    "srt_set_gather_planes": (_i, [_vp, _u32]),
    "srt_tile_buffer": (_i, [_vp, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_u32), C.POINTER(_u32)]),
    "srt_copy_tile_buffer": (_i, [_vp, _vp, _vp]),
    "srt_scatter_tiles": (_i, [_vp, _vp, _vp]),
    "srt_accum_exchange_size": (_i, [_vp, _u32, C.POINTER(_sz)]),
    "srt_pack_accum": (_i, [_vp, _u32, _vp, _vp]),
    "srt_unpack_accum": (_i, [_vp, _u32, _vp, _vp]),
    "srt_accum_gathered": (_i, [_vp, C.POINTER(_u32)]),
    "srt_accum_whole": (_i, [_vp, _u32, C.POINTER(_i)]),
    "srt_gather_last_ms": (_i, [_vp, _fp, _fp]),
    "srt_dev_fb": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz)]),
    "srt_read_fb": (_i, [_vp, _fp, _fp, _fp]),
    "srt_read_fb_rowmajor": (_i, [_vp, _fp, _fp, _fp, _u32, _u32]),
    "srt_read_fb_aux": (_i, [_vp, _i, _fp, _fp, _fp]),
    "srt_get_tile_costs": (_i, [_vp, C.POINTER(C.c_uint32), _sz]),
    "srt_order_children_by_profile": (_i, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "srt_pixels_per_lane": (_i, [_vp, _u32, _u32, _u32, C.POINTER(C.c_double)]),
    "srt_tune_tree_for_throughput": (_i, [_vp, _vp, _u32, _u32, _u32, _u32, _i, C.POINTER(TreeTuning)]),
    "srt_tune_tree_with_segments": (_i, [_vp, _vp, _u32, _u32, _u32, _u32, _i, _fp, _sz, C.POINTER(TreeTuning)]),
    "srt_collect_ray_segments": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u64, _fp, _sz, C.POINTER(_sz), C.POINTER(_u64)]),
    "srt_get_stats": (_i, [_vp, C.POINTER(Stats)]),
    "srt_set_count_traversal": (_i, [_vp, _i]),
    "srt_get_wave_debug": (_i, [_vp, C.POINTER(C.c_uint32), _sz]),
    "srt_last_kernel_ms": (_i, [_vp, C.POINTER(_f)]),
    "srt_trace_rays": (_i, [_vp, _fp, _sz, _fp]),
    "srt_intersect_rays": (_i, [_vp, _fp, _sz, _fp]),
    "srt_occluded_rays": (_i, [_vp, _fp, _sz, C.POINTER(C.c_uint8)]),
    "srt_intersect_rays_dev": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "srt_occluded_rays_dev": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "srt_query_last": (_i, [_vp, C.POINTER(QueryInfo)]),
    "srt_set_query_test_grid": (_i, [_vp, _u32]),
    "srt_direct_light": (_i, [_vp, C.POINTER(Light), _fp, _fp, C.POINTER(LightResult), _u32, _u32, _u32, _u32]),
    "srt_direct_light_kat": (_i, [_vp, C.POINTER(Light), _fp, _fp, C.POINTER(LightResult), _u32, _u32, _u32, _u32, _fp, _fp, _fp, _fp,
                                  C.POINTER(_u32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "srt_read_light_table": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32), _fp, _sz]),
    "srt_direct_light_last": (_i, [_vp, C.POINTER(LightInfo)]),
    "srt_set_light_test_batch": (_i, [_vp, _u32]),
    "srt_device_op_sweep": (_i, [_vp, _i, _fp, _fp, _sz, _fp]),
    "srt_order_tiles_kat": (_i, [_vp, C.POINTER(_u32), _u32, _u32, _u32, _u32, C.POINTER(_u32), _sz, C.POINTER(_u32), C.POINTER(_u32)]),
    "srt_read_tile_schedule": (_i, [_vp, _i, C.POINTER(_u32), _sz, C.POINTER(TileScheduleInfo)]),
    "srt_calibrate": (_i, [_vp, _i, _u32, _u32, C.POINTER(Calibration)]),
    "srt_ctx_device": (_i, [_vp]),
    "srt_ctx_cu_count": (_i, [_vp]),
    "srt_comm_init_all": (_i, [C.POINTER(_i), _i, C.POINTER(_vp)]),
    "srt_comm_unique_id": (_i, [C.POINTER(C.c_ubyte)]),
    "srt_comm_init_rank": (_i, [_vp, C.POINTER(C.c_ubyte), _u32, _u32, C.POINTER(_vp)]),
    "srt_comm_available": (_i, []),
    "srt_comm_set_gather_planes": (_i, [_vp, _u32]),
    "srt_comm_last_gather_ms": (_i, [_vp, C.POINTER(_f)]),
    "srt_comm_gather_accum": (_i, [_vp, _u32]),
    "srt_comm_last_accum_gather_ms": (_i, [_vp, _fp, _fp, _fp]),
    "srt_comm_destroy": (None, [_vp]),
    "srt_comm_last_error": (C.c_char_p, [_vp]),
    "srt_comm_world": (_u32, [_vp]),
    "srt_comm_local_count": (_u32, [_vp]),
    "srt_comm_ctx": (_vp, [_vp, _u32]),
    "srt_comm_root_ctx": (_vp, [_vp]),
    "srt_comm_upload_scene": (_i, [_vp, _vp]),
    "srt_comm_refit_vertices": (_i, [_vp, _fp, _sz]),
    "srt_comm_set_camera": (_i, [_vp, C.POINTER(CameraData)]),
    "srt_comm_init_device_params": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _u64]),
    "srt_render_frame_multi": (_i, [_vp, _u32, _u32, _u32, _u32]),
    "srt_comm_accum_reset": (_i, [_vp]),
    "srt_render_frame_multi_accum": (_i, [_vp, _u32, _u32, _u32, _u32, _u32]),
    "srt_comm_accum_reset_adaptive": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_comm_accum_active": (_i, [_vp, C.POINTER(_u64)]),
    "srt_comm_accum_reset_spectral": (_i, [_vp]),
    "srt_comm_accum_reset_features": (_i, [_vp]),
    "srt_comm_accum_reset_adaptive_features": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_comm_accum_reset_spectral_features": (_i, [_vp]),
    "srt_comm_accum_reset_adaptive_spectral": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_comm_accum_reset_adaptive_spectral_features": (_i, [_vp, C.POINTER(Adaptive)]),
    "srt_comm_accum_reset_streams": (_i, [_vp, _u32]),
    "srt_comm_synchronize": (_i, [_vp]),
    "srt_comm_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_f)]),
}


class SrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("srt error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load libsrt_hip.so (built in-tree by __graft_entry__.build()).  No fallback: raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the render path)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)          # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


COMM_ID_BYTES = 128


def check_comm(code, comm=None):
    if code is not None and code < 0:
        msg = lib().srt_comm_last_error(comm)
        raise SrtError(code, msg.decode() if msg else "")
    return code


def check(code, ctx=None):
    if code is not None and code < 0:
        msg = lib().srt_last_error(ctx)
        raise SrtError(code, msg.decode() if msg else "")
    return code


def fptr(arr):
    """float32 C-contiguous numpy array -> float*"""
    return arr.ctypes.data_as(_fp)
