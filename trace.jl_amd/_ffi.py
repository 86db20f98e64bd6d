"""ctypes binding of libtracehip.so (include/tracehip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is no CPU fallback: if the shared
object is missing or no MI355X is visible, the entry points raise ``TraceHipError`` — they never route through oracle/.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRHIP_LIB", os.path.join(_HERE, "libtracehip.so"))  # TRHIP_LIB: A/B builds for tuning (tools/)


class TraceHipError(RuntimeError):
    pass


class Sensor(C.Structure):
    """trhip_sensor"""
    _fields_ = [
        ("raster_to_camera", C.c_float * 16),
        ("camera_to_world", C.c_float * 16),
        ("lens_radius", C.c_float),
        ("focal_distance", C.c_float),
        ("shutter_open", C.c_float),
        ("shutter_close", C.c_float),
        ("crop_min", C.c_float * 2),
        ("crop_max", C.c_float * 2),
        ("filter_radius", C.c_float * 2),
        ("filter_table", C.c_float * 256),
        ("scale", C.c_float),
    ]


class Stats(C.Structure):
    """trhip_stats"""
    _fields_ = [
        ("camera_samples", C.c_uint64),
        ("closest_rays", C.c_uint64),
        ("shadow_rays", C.c_uint64),
        ("nodes_visited", C.c_uint64),
        ("prims_tested", C.c_uint64),
        ("nodes_visited_shadow", C.c_uint64),
        ("prims_tested_shadow", C.c_uint64),
        ("ms_total", C.c_double),
        ("ms_raygen", C.c_double),
        ("ms_trace_closest", C.c_double),
        ("ms_shade", C.c_double),
        ("ms_trace_any", C.c_double),
        ("ms_film", C.c_double),
        ("launches_raygen", C.c_uint32),
        ("launches_trace_closest", C.c_uint32),
        ("launches_shade", C.c_uint32),
        ("launches_trace_any", C.c_uint32),
        ("launches_film", C.c_uint32),
        ("n_batches", C.c_uint32),
        ("max_depth_reached", C.c_uint32),
        ("traversal", C.c_uint32),
        ("node_bytes", C.c_uint32),
        ("replicated_rays", C.c_uint64),
        ("fallback_rays", C.c_uint64),
        ("ms_sub", C.c_double * 4),
        ("launches_sub", C.c_uint32 * 4),
        ("count_sub", C.c_uint64 * 4),
        ("ms_fallback", C.c_double),
        ("launches_fallback", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("nodes_visited_fallback", C.c_uint64),
        ("prims_tested_fallback", C.c_uint64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


UNIQUE_ID_BYTES = 128  # TRHIP_UNIQUE_ID_BYTES


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: rank 0 calls this and hands the 128 bytes to the other processes."""
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    rc = lib().trhip_comm_unique_id(buf)
    if rc:
        raise TraceHipError(f"trhip_comm_unique_id failed ({rc}): {lib().trhip_last_error(None).decode()}")
    return bytes(buf)


HIT_DTYPE = np.dtype([("t", np.float32), ("prim", np.int32), ("b1", np.float32), ("b2", np.float32)])


class AovSample(C.Structure):
    """trhip_aov_sample: one camera sample of a feature-buffer frame (80 bytes, five 16-byte words)"""
    _fields_ = [
        ("t", C.c_float),
        ("prim", C.c_int32),
        ("b1", C.c_float),
        ("b2", C.c_float),
        ("p", C.c_float * 3),
        ("material", C.c_int32),
        ("n", C.c_float * 3),
        ("pad0", C.c_uint32),
        ("ns", C.c_float * 3),
        ("pad1", C.c_uint32),
        ("albedo", C.c_float * 3),
        ("pad2", C.c_uint32),
    ]


# the same record as a numpy structured dtype (AOVIntegrator.samples)
AOV_DTYPE = np.dtype([("t", np.float32), ("prim", np.int32), ("b1", np.float32), ("b2", np.float32), ("p", np.float32, 3), ("material", np.int32), ("n", np.float32, 3), ("pad0", np.uint32),
                      ("ns", np.float32, 3), ("pad1", np.uint32), ("albedo", np.float32, 3), ("pad2", np.uint32)])


class DenoiseParams(C.Structure):
    """trhip_denoise_params (32 bytes)"""
    _fields_ = [
        ("iterations", C.c_uint32),
        ("flags", C.c_uint32),
        ("sigma_colour", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_plane", C.c_float),
        ("albedo_floor", C.c_float),
        ("min_coverage", C.c_float),
        ("reserved", C.c_uint32),
    ]


DENOISE_DEMODULATE = 1  # TRHIP_DENOISE_DEMODULATE


class SampleMapParams(C.Structure):
    """trhip_sample_map_params (24 bytes)"""
    _fields_ = [
        ("tau", C.c_float),
        ("eps", C.c_float),
        ("pilot", C.c_uint32),
        ("max_extra", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class AoParams(C.Structure):
    """trhip_ao_params (16 bytes)"""
    _fields_ = [
        ("max_distance", C.c_float),
        ("background", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


AO_ALBEDO = 1  # TRHIP_AO_ALBEDO


class SkyParams(C.Structure):
    """trhip_sky_params (16 bytes)"""
    _fields_ = [
        ("max_distance", C.c_float),
        ("scale", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


SKY_ALBEDO = 1  # TRHIP_SKY_ALBEDO
SKY_HIDE_BACKGROUND = 2  # TRHIP_SKY_HIDE_BACKGROUND
ENV_MAX_N = 4096  # the largest map trhip_env_create takes


class SkyIsParams(C.Structure):
    """trhip_sky_is_params (32 bytes)"""
    _fields_ = [
        ("max_distance", C.c_float),
        ("scale", C.c_float),
        ("mix", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class PathEnvParams(C.Structure):
    """trhip_path_env_params (16 bytes)"""
    _fields_ = [
        ("scale", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


PATH_ENV_HIDE_BACKGROUND = 1  # TRHIP_PATH_ENV_HIDE_BACKGROUND


class PathNeeParams(C.Structure):
    """trhip_path_nee_params (32 bytes)"""
    _fields_ = [
        ("scale", C.c_float),
        ("mix", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 5),
    ]


class PathEmitParams(C.Structure):
    """trhip_path_emit_params (32 bytes)"""
    _fields_ = [
        ("scale", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 6),
    ]


PATH_EMIT_HITS_ONLY = 1  # TRHIP_PATH_EMIT_HITS_ONLY


class TemporalParams(C.Structure):
    """trhip_temporal_params (72 bytes)"""
    _fields_ = [
        ("prev_world_to_pixel", C.c_float * 12),
        ("max_history", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_plane", C.c_float),
        ("min_coverage", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class TemporalClipParams(C.Structure):
    """trhip_temporal_clip_params (88 bytes)"""
    _fields_ = [
        ("base", TemporalParams),
        ("clip_gamma", C.c_float),
        ("clip_radius", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class TemporalMomentsParams(C.Structure):
    """trhip_temporal_moments_params (88 bytes)"""
    _fields_ = [
        ("base", TemporalParams),
        ("albedo_floor", C.c_float),
        ("spatial_below", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class DenoiseVarParams(C.Structure):
    """trhip_denoise_var_params (48 bytes)"""
    _fields_ = [
        ("base", DenoiseParams),
        ("var_eps", C.c_float),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class UpscaleParams(C.Structure):
    """trhip_upscale_params (48 bytes)"""
    _fields_ = [
        ("lo_from_hi", C.c_float * 4),
        ("radius", C.c_uint32),
        ("flags", C.c_uint32),
        ("sigma_normal", C.c_float),
        ("sigma_plane", C.c_float),
        ("albedo_floor", C.c_float),
        ("min_coverage", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


UPSCALE_DEMODULATE = 1  # TRHIP_UPSCALE_DEMODULATE
UPSCALE_COVERAGE = 2    # TRHIP_UPSCALE_COVERAGE


class TemporalUpsampleParams(C.Structure):
    """trhip_temporal_upsample_params (112 bytes)"""
    _fields_ = [
        ("lo_from_hi", C.c_float * 4),
        ("prev_world_to_pixel", C.c_float * 12),
        ("max_history", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_plane", C.c_float),
        ("min_coverage", C.c_float),
        ("guide_sigma_normal", C.c_float),
        ("guide_sigma_plane", C.c_float),
        ("confidence_floor", C.c_float),
        ("confidence_sharpness", C.c_float),
        ("radius", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class TemporalMotionParams(C.Structure):
    """trhip_temporal_motion_params (80 bytes)"""
    _fields_ = [
        ("prev_world_to_pixel", C.c_float * 12),
        ("max_history", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_plane", C.c_float),
        ("min_coverage", C.c_float),
        ("n_prims", C.c_uint32),
        ("n_bodies", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class TemporalUpsampleMotionParams(C.Structure):
    """trhip_temporal_upsample_motion_params (128 bytes)"""
    _fields_ = [
        ("base", TemporalUpsampleParams),
        ("n_prims", C.c_uint32),
        ("n_bodies", C.c_uint32),
        ("motion_flags", C.c_uint32),
        ("reserved2", C.c_uint32),
    ]


class TemporalClipMotionParams(C.Structure):
    """trhip_temporal_clip_motion_params (96 bytes)"""
    _fields_ = [
        ("base", TemporalMotionParams),
        ("clip_gamma", C.c_float),
        ("clip_radius", C.c_uint32),
        ("clip_max_history", C.c_float),
        ("reserved2", C.c_uint32),
    ]


# trhip_aov_id, the record of the id plane (AOVIntegrator.ids)
AOV_ID_DTYPE = np.dtype([("prim", np.int32), ("material", np.int32), ("t", np.float32), ("n_hit", np.uint32)])
STATIC_BODY = 0xFFFFFFFF  # the conventional "no body" word of body_of_prim


class DisplayParams(C.Structure):
    """trhip_display_params (48 bytes)"""
    _fields_ = [
        ("curve", C.c_uint32),
        ("transfer", C.c_uint32),
        ("flags", C.c_uint32),
        ("exposure", C.c_float),
        ("key", C.c_float),
        ("percentile_permille", C.c_uint32),
        ("adapt_rate", C.c_float),
        ("min_exposure", C.c_float),
        ("max_exposure", C.c_float),
        ("white", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


class DisplayState(C.Structure):
    """trhip_display_state (16 bytes); all zero = no state"""
    _fields_ = [("exposure", C.c_float), ("valid", C.c_uint32), ("counted", C.c_uint32), ("key_bin", C.c_uint32)]


DISPLAY_AUTO_EXPOSURE = 1  # TRHIP_DISPLAY_AUTO_EXPOSURE
DISPLAY_FLIP_ROWS = 2      # TRHIP_DISPLAY_FLIP_ROWS
DISPLAY_CURVES = {"clamp": 0, "reinhard": 1, "aces": 2}  # TRHIP_DISPLAY_CURVE_*
DISPLAY_TRANSFERS = {"linear": 0, "srgb": 1}             # TRHIP_DISPLAY_TRANSFER_*

_F = C.POINTER(C.c_float)
_U32 = C.POINTER(C.c_uint32)
_VP = C.c_void_p
SPPM_WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_float))  # trhip_sppm_write_fn

# name -> (restype, argtypes); every symbol include/tracehip.h declares
SIGNATURES = {
    "trhip_version": (C.c_int, []),
    "trhip_init": (C.c_int, [C.POINTER(_VP), C.c_int]),
    "trhip_shutdown": (None, [_VP]),
    "trhip_last_error": (C.c_char_p, [_VP]),
    "trhip_scene_new": (C.c_int, [_VP, C.POINTER(_VP)]),
    "trhip_scene_free": (None, [_VP]),
    "trhip_scene_add_material": (C.c_int, [_VP, C.c_int, _F, C.c_int, _U32]),
    "trhip_scene_add_triangles": (C.c_int, [_VP, _F, C.c_uint32, _U32, C.c_uint32, _F, _U32, C.c_int, _U32]),
    "trhip_scene_add_triangles_ex": (C.c_int, [_VP, _F, C.c_uint32, _U32, C.c_uint32, _F, _F, _F, _U32, C.c_int, _U32]),
    "trhip_scene_add_sphere": (C.c_int, [_VP, _F, _F, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, _U32]),
    "trhip_scene_add_sphere_fields": (C.c_int, [_VP, _F, _F, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, _U32]),
    "trhip_scene_add_spot_light_fields": (C.c_int, [_VP, _F, _F, _F, C.c_float, C.c_float]),
    "trhip_scene_add_point_light": (C.c_int, [_VP, _F, _F, _F]),
    "trhip_scene_add_spot_light": (C.c_int, [_VP, _F, _F, _F, C.c_float, C.c_float]),
    "trhip_scene_add_directional_light": (C.c_int, [_VP, _F, _F, C.c_float]),
    "trhip_scene_commit": (C.c_int, [_VP, C.c_int]),
    "trhip_scene_relight": (C.c_int, [_VP, C.POINTER(_VP)]),
    "trhip_scene_geometry_id": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "trhip_build_bvh_host": (C.c_int, [C.c_int, _F, C.c_uint32, C.c_int, _F, _U32, _U32, _U32, _U32, _U32]),
    "trhip_scene_bvh_size": (C.c_int, [_VP, _U32, _U32]),
    "trhip_scene_get_bvh": (C.c_int, [_VP, _F, _U32, _U32, _U32]),
    "trhip_scene_set_bvh": (C.c_int, [_VP, _F, _U32, _U32, C.c_uint32, _U32, C.c_uint32]),
    "trhip_plan_bands": (C.c_int, [C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, _U32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "trhip_scene_bvh_mode": (C.c_int, [_VP, C.POINTER(C.c_int), _U32, _U32]),
    "trhip_scene_bvh_note": (C.c_int, [_VP, C.c_char_p, C.c_size_t]),
    "trhip_scene_get_accelerator": (C.c_int, [_VP, _F, _U32, _U32, _U32]),
    "trhip_render_whitted": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _F, C.POINTER(Stats)]),
    "trhip_render_path": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _F, C.POINTER(Stats)]),
    "trhip_render_path_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(Stats)]),
    "trhip_render_whitted_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(Stats)]),
    "trhip_last_sample_radiance": (C.c_int, [_VP, _F, C.c_uint64]),
    "trhip_render_path_map": (C.c_int, [_VP, _VP, C.POINTER(Sensor), _U32, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _F, C.POINTER(Stats)]),
    "trhip_render_path_map_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), _VP, C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(Stats)]),
    "trhip_film_sum": (C.c_int, [_VP, _F, _F, C.c_uint32, C.c_uint32, _F]),
    "trhip_film_sum_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, _VP]),
    "trhip_last_sample_stats": (C.c_int, [_VP, _F]),
    "trhip_last_sample_stats_device": (C.c_int, [_VP, _VP]),
    "trhip_sample_map_default_params": (C.c_int, [C.POINTER(SampleMapParams)]),
    "trhip_sample_map": (C.c_int, [_VP, _F, C.c_uint32, C.c_uint32, C.POINTER(SampleMapParams), _U32, C.POINTER(C.c_uint64)]),
    "trhip_sample_map_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(SampleMapParams), _VP, _VP]),
    "trhip_render_aov": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _F, _VP, C.POINTER(Stats)]),
    "trhip_render_aov_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _VP, _VP, C.POINTER(Stats)]),
    "trhip_ao_default_params": (C.c_int, [C.POINTER(AoParams)]),
    "trhip_render_ao": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(AoParams), _F, C.POINTER(Stats)]),
    "trhip_render_ao_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(AoParams), _VP, C.POINTER(Stats)]),
    "trhip_denoise_default_params": (C.c_int, [C.POINTER(DenoiseParams)]),
    "trhip_denoise": (C.c_int, [_VP, _F, _F, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), _F, C.POINTER(Stats)]),
    "trhip_denoise_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(DenoiseParams), _VP, C.POINTER(Stats)]),
    "trhip_sensor_world_to_pixel": (C.c_int, [C.POINTER(Sensor), _F]),
    "trhip_temporal_default_params": (C.c_int, [C.POINTER(TemporalParams)]),
    "trhip_temporal": (C.c_int, [_VP, _F, _F, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalParams), _F, _F, C.POINTER(Stats)]),
    "trhip_temporal_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(TemporalParams), _VP, _VP, C.POINTER(Stats)]),
    "trhip_temporal_clip_default_params": (C.c_int, [C.POINTER(TemporalClipParams)]),
    "trhip_temporal_clip": (C.c_int, [_VP, _F, _F, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalClipParams), _F, _F, C.POINTER(Stats)]),
    "trhip_temporal_clip_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(TemporalClipParams), _VP, _VP, C.POINTER(Stats)]),
    "trhip_temporal_moments_default_params": (C.c_int, [C.POINTER(TemporalMomentsParams)]),
    "trhip_temporal_moments": (C.c_int, [_VP, _F, _F, _F, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalMomentsParams), _F, _F, _F, _F, C.POINTER(Stats)]),
    "trhip_temporal_moments_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(TemporalMomentsParams), _VP, _VP, _VP, _VP, C.POINTER(Stats)]),
    "trhip_denoise_var_default_params": (C.c_int, [C.POINTER(DenoiseVarParams)]),
    "trhip_denoise_var": (C.c_int, [_VP, _F, _F, _F, C.c_uint32, C.c_uint32, C.POINTER(DenoiseVarParams), _F, _F, C.POINTER(Stats)]),
    "trhip_denoise_var_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(DenoiseVarParams), _VP, _VP, C.POINTER(Stats)]),
    "trhip_upscale_default_params": (C.c_int, [C.POINTER(UpscaleParams)]),
    "trhip_upscale": (C.c_int, [_VP, _F, _F, C.c_uint32, C.c_uint32, _F, C.c_uint32, C.c_uint32, C.POINTER(UpscaleParams), _F, C.POINTER(C.c_uint8), C.POINTER(Stats)]),
    "trhip_upscale_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, _VP, C.c_uint32, C.c_uint32, C.POINTER(UpscaleParams), _VP, _VP, C.POINTER(Stats)]),
    "trhip_display_default_params": (C.c_int, [C.POINTER(DisplayParams)]),
    "trhip_display_srgb_table": (C.c_int, [_F]),
    "trhip_display": (C.c_int, [_VP, _F, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(DisplayParams), C.POINTER(DisplayState), C.POINTER(C.c_uint8), _U32, C.POINTER(Stats)]),
    "trhip_display_device": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(DisplayParams), _VP, _VP, _VP, C.POINTER(Stats)]),
    "trhip_temporal_upsample_default_params": (C.c_int, [C.POINTER(TemporalUpsampleParams)]),
    "trhip_temporal_upsample": (C.c_int, [_VP, _F, _F, C.c_uint32, C.c_uint32, _F, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalUpsampleParams), _F, _F, C.POINTER(C.c_uint8),
                                          C.POINTER(Stats)]),
    "trhip_temporal_upsample_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(TemporalUpsampleParams), _VP, _VP, _VP,
                                                 C.POINTER(Stats)]),
    "trhip_env_create": (C.c_int, [_VP, _F, C.c_uint32, _F, C.POINTER(_VP)]),
    "trhip_env_free": (None, [_VP]),
    "trhip_env_size": (C.c_int, [_VP, _U32]),
    "trhip_env_eval": (C.c_int, [_VP, _VP, _F, C.c_uint64, _F]),
    "trhip_sky_default_params": (C.c_int, [C.POINTER(SkyParams)]),
    "trhip_render_sky": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _VP, C.POINTER(SkyParams), _F, C.POINTER(Stats)]),
    "trhip_render_sky_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _VP, C.POINTER(SkyParams), _VP, C.POINTER(Stats)]),
    "trhip_env_make_sampler": (C.c_int, [_VP, _VP]),
    "trhip_env_sample": (C.c_int, [_VP, _VP, _F, C.c_uint64, _F]),
    "trhip_env_pdf": (C.c_int, [_VP, _VP, _F, C.c_uint64, _F]),
    "trhip_sky_is_default_params": (C.c_int, [C.POINTER(SkyIsParams)]),
    "trhip_render_sky_is": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _VP, C.POINTER(SkyIsParams), _F, C.POINTER(Stats)]),
    "trhip_render_sky_is_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _VP, C.POINTER(SkyIsParams), _VP, C.POINTER(Stats)]),
    "trhip_path_env_default_params": (C.c_int, [C.POINTER(PathEnvParams)]),
    "trhip_render_path_env": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(PathEnvParams), _F, C.POINTER(Stats)]),
    "trhip_render_path_env_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(PathEnvParams), _VP, C.POINTER(Stats)]),
    "trhip_last_escapes": (C.c_int, [_VP, _F, C.c_uint64]),
    "trhip_path_nee_default_params": (C.c_int, [C.POINTER(PathNeeParams)]),
    "trhip_render_path_env_nee": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(PathNeeParams), _F, C.POINTER(Stats)]),
    "trhip_render_path_env_nee_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(PathNeeParams), _VP, C.POINTER(Stats)]),
    "trhip_emitters_create": (C.c_int, [_VP, _VP, C.POINTER(C.c_uint32), _F, C.c_uint32, C.POINTER(_VP)]),
    "trhip_emitters_free": (None, [_VP]),
    "trhip_emitters_size": (C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    "trhip_emitters_sample": (C.c_int, [_VP, _VP, _F, C.c_uint64, C.POINTER(C.c_uint32), _F, _F]),
    "trhip_path_emit_default_params": (C.c_int, [C.POINTER(PathEmitParams)]),
    "trhip_render_path_emit": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(PathEmitParams), _F, C.POINTER(Stats)]),
    "trhip_render_path_emit_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _VP, C.POINTER(PathEmitParams), _VP, C.POINTER(Stats)]),
    "trhip_last_emitted": (C.c_int, [_VP, _F, C.c_uint64]),
    "trhip_path_env_relight": (C.c_int, [_VP, _VP, C.POINTER(PathEnvParams), _F]),
    "trhip_path_env_relight_device": (C.c_int, [_VP, _VP, C.POINTER(PathEnvParams), _VP]),
    "trhip_render_aov_ids": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _F, _VP, _VP, C.POINTER(Stats)]),
    "trhip_render_aov_ids_device": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _VP, _VP, _VP, C.POINTER(Stats)]),
    "trhip_temporal_motion_default_params": (C.c_int, [C.POINTER(TemporalMotionParams)]),
    "trhip_temporal_motion": (C.c_int, [_VP, _F, _F, _F, _VP, _U32, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalMotionParams), _F, _F, C.POINTER(Stats)]),
    "trhip_temporal_motion_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(TemporalMotionParams), _VP, _VP, C.POINTER(Stats)]),
    "trhip_temporal_clip_motion_default_params": (C.c_int, [C.POINTER(TemporalClipMotionParams)]),
    "trhip_temporal_clip_motion": (C.c_int, [_VP, _F, _F, _F, _VP, _U32, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalClipMotionParams), _F, _F, C.POINTER(Stats)]),
    "trhip_temporal_clip_motion_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(TemporalClipMotionParams), _VP, _VP, C.POINTER(Stats)]),
    "trhip_temporal_upsample_motion_default_params": (C.c_int, [C.POINTER(TemporalUpsampleMotionParams)]),
    "trhip_temporal_upsample_motion": (C.c_int, [_VP, _F, _F, C.c_uint32, C.c_uint32, _F, _F, _VP, _U32, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalUpsampleMotionParams), _F, _F,
                                                 C.POINTER(C.c_uint8), C.POINTER(Stats)]),
    "trhip_temporal_upsample_motion_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, _VP, _VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32,
                                                        C.POINTER(TemporalUpsampleMotionParams), _VP, _VP, _VP, C.POINTER(Stats)]),
    "trhip_temporal_split": (C.c_int, [_VP, _F, _F, _F, _F, _VP, _U32, _F, C.c_uint32, C.c_uint32, C.POINTER(TemporalMotionParams), _F, _F, C.POINTER(Stats)]),
    "trhip_temporal_split_device": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint32, C.c_uint32, C.POINTER(TemporalMotionParams), _VP, _VP, C.POINTER(Stats)]),
    "trhip_film_add": (C.c_int, [_VP, _F, _F, C.c_uint32, C.c_uint32, _F, C.POINTER(Stats)]),
    "trhip_film_add_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, _VP, C.POINTER(Stats)]),
    "trhip_render_sppm": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_float, C.c_int, C.c_uint32, C.c_int64, C.c_uint64, _F, C.POINTER(Stats)]),
    "trhip_render_sppm_ex": (C.c_int, [_VP, _VP, C.POINTER(Sensor), C.c_float, C.c_int, C.c_uint32, C.c_int64, C.c_uint64, _F, C.POINTER(Stats), C.c_uint32, SPPM_WRITE_FN, _VP]),
    "trhip_sppm_state": (C.c_int, [_VP, _F, _F, _F, C.POINTER(C.c_double), C.POINTER(C.c_int64), _F, _F, _F, C.POINTER(C.c_int64)]),
    "trhip_film_to_rgb": (C.c_int, [_VP, _F, C.c_uint32, C.c_uint32, C.c_float, _F]),
    "trhip_trace_closest": (C.c_int, [_VP, _VP, _F, C.c_uint64, _VP]),
    "trhip_trace_any": (C.c_int, [_VP, _VP, _F, C.c_uint64, C.POINTER(C.c_uint8)]),
    "trhip_trace_closest_device": (C.c_int, [_VP, _VP, _VP, C.c_uint64, _VP, C.c_int, C.POINTER(C.c_double)]),
    "trhip_trace_any_device": (C.c_int, [_VP, _VP, _VP, C.c_uint64, _VP, C.c_int, C.POINTER(C.c_double)]),
    "trhip_accelerator_note": (C.c_int, [_VP, _VP, C.c_char_p, C.c_size_t]),
    "trhip_last_visit_counts": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "trhip_last_fallback_counts": (C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    "trhip_last_bvh_build_ms": (C.c_int, [_VP, C.POINTER(C.c_double)]),
    "trhip_hit_geometry": (C.c_int, [_VP, _VP, _F, C.c_uint64, _F]),
    "trhip_generate_rays": (C.c_int, [_VP, C.POINTER(Sensor), _F, C.c_uint64, _F]),
    "trhip_bsdf_query": (C.c_int, [_VP, _VP, C.c_uint32, C.c_int, C.c_int, C.c_int, _F, _F, C.c_uint64, _F]),
    "trhip_film_accumulate": (C.c_int, [_VP, C.POINTER(Sensor), C.c_uint32, C.c_uint64, C.c_uint32, _F, _F]),
    "trhip_set_option": (C.c_int, [_VP, C.c_char_p, C.c_int64]),
    "trhip_option_in_build": (C.c_int, [C.c_char_p, C.c_int64]),
    "trhip_closest_kernel_name": (C.c_int, [_VP, _VP, C.c_char_p, C.c_size_t]),
    "trhip_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "trhip_comm_init": (C.c_int, [_VP, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    "trhip_comm_destroy": (C.c_int, [_VP]),
    "trhip_comm_rank": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "trhip_film_reduce": (C.c_int, [_VP, _VP, C.c_uint64, C.c_int]),
    "trhip_film_allreduce": (C.c_int, [_VP, _VP, C.c_uint64]),
    "trhip_detmath_f32": (C.c_int, [C.c_int, _F, _F, C.c_uint64, _F]),
    "trhip_detmath_f32_device": (C.c_int, [_VP, C.c_int, _F, _F, C.c_uint64, _F]),
}

_lib = None


def lib():
    """Load libtracehip.so (once) and attach the prototypes.  Loading needs no GPU; computing does."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TraceHipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def fptr(a):
    return a.ctypes.data_as(_F)


def u32ptr(a):
    return a.ctypes.data_as(_U32)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


_POINTER_OF = {np.dtype(np.float32): _F, np.dtype(np.uint32): _U32, np.dtype(np.uint8): C.POINTER(C.c_uint8)}


def optr(a):
    """An optional host array for a call: None stays None (NULL); a Float32, UInt32 or UInt8 array gives the pointer of its element type, any other (the 16-byte
    records of an id plane) a void *."""
    return None if a is None else a.ctypes.data_as(_POINTER_OF.get(a.dtype, _VP))


def dptr(p):
    """An optional device address for a call: None or 0 stays None (NULL)."""
    return _VP(p) if p else None


def default_params(struct_type, entry_name: str):
    """A parameter block filled by its trhip_*_default_params entry (host arithmetic: no context, no GPU)."""
    p = struct_type()
    rc = getattr(lib(), entry_name)(C.byref(p))
    if rc:
        raise TraceHipError(f"{entry_name} failed ({rc})")
    return p


def build_bvh_host(prim_bounds, max_node_primitives: int = 1, builder: int = 2):
    """BVHAccel construction alone, on the host (trhip_build_bvh_host; no GPU needed): builder 2 = the reference's own construction node for
    node (accel/bvh.jl:87-206), 0 = the library's binned SAH.  prim_bounds: (n, 6) world bounds.  Returns (bounds (m, 6), a, flags, order, max_depth)
    in the layout of FlatScene.bvh() / set_bvh()."""
    import numpy as np
    pb = f32(prim_bounds).reshape(-1, 6)
    n_nodes, depth = C.c_uint32(0), C.c_uint32(0)

    def check(rc):
        if rc:
            raise TraceHipError(f"trhip_build_bvh_host failed ({rc}): {lib().trhip_last_error(None).decode()}")
    check(lib().trhip_build_bvh_host(builder, fptr(pb), pb.shape[0], max_node_primitives, None, None, None, C.byref(n_nodes), None, C.byref(depth)))
    m = n_nodes.value
    bounds, a, flags, order = np.empty((m, 6), np.float32), np.empty(m, np.uint32), np.empty(m, np.uint32), np.empty(pb.shape[0], np.uint32)
    check(lib().trhip_build_bvh_host(builder, fptr(pb), pb.shape[0], max_node_primitives, fptr(bounds), u32ptr(a), u32ptr(flags), C.byref(n_nodes), u32ptr(order), C.byref(depth)))
    return bounds, a, flags, order, depth.value


def detmath(fn: int, x, y=None):
    """Deterministic Float32 elementary functions (include/trace_detmath.h), evaluated by the library on the host."""
    x = f32(np.atleast_1d(x))
    out = np.empty_like(x)
    yy = f32(np.atleast_1d(y)) if y is not None else None
    rc = lib().trhip_detmath_f32(fn, fptr(x), optr(yy), x.size, fptr(out))
    if rc:
        raise TraceHipError("trhip_detmath_f32 failed")
    return out


class Context:
    """One GPU (trhip_ctx)."""

    def detmath(self, fn: int, x, y=None):
        """include/trace_detmath.h evaluated by a kernel on this GPU (trhip_detmath_f32_device)."""
        x = f32(np.atleast_1d(x))
        out = np.empty_like(x)
        yy = f32(np.atleast_1d(y)) if y is not None else None
        self.check(lib().trhip_detmath_f32_device(self._h, fn, fptr(x), optr(yy), x.size, fptr(out)))
        return out

    def __init__(self, device: int = 0):
        self._h = _VP()
        rc = lib().trhip_init(C.byref(self._h), device)
        if rc:
            msg = lib().trhip_last_error(None).decode()
            self._h = None
            raise TraceHipError(f"trhip_init failed ({rc}): {msg}")

    def check(self, rc):
        if rc:
            raise TraceHipError(f"libtracehip error {rc}: {lib().trhip_last_error(self._h).decode()}")

    def set_option(self, name: str, value: int):
        self.check(lib().trhip_set_option(self._h, name.encode(), int(value)))

    def has_option(self, name: str, value: int) -> bool:
        """Whether this build of the library honours the option value (the kernel families that lost their measurements — traversals 4 / 6 / 7, leaf_queue, leaf_sorted,
        the linear BVH builder — exist only in the EXPERIMENTS build: __graft_entry__.build_library(extra_flags=["-DTRHIP_EXPERIMENTS"], …)).  The option is left as it was
        when the answer is no, and SET when it is yes."""
        return lib().trhip_set_option(self._h, name.encode(), int(value)) != -3

    # ---- multi-GPU job (include/tracehip.h "multi-GPU"): one process per GPU, RCCL behind the C ABI -------------------
    def comm_init(self, unique_id: bytes, rank: int, n_ranks: int):
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self.check(lib().trhip_comm_init(self._h, buf, int(rank), int(n_ranks)))

    def comm_destroy(self):
        self.check(lib().trhip_comm_destroy(self._h))

    def comm_rank(self):
        r, n = C.c_int(), C.c_int()
        self.check(lib().trhip_comm_rank(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def film_reduce(self, device_ptr: int, n_pixels: int, root: int = 0):
        """In-place sum of the (H, W, 4) film accumulators of all ranks onto `root` (ncclReduce inside the library)."""
        self.check(lib().trhip_film_reduce(self._h, C.c_void_p(int(device_ptr)), int(n_pixels), int(root)))

    def film_allreduce(self, device_ptr: int, n_pixels: int):
        self.check(lib().trhip_film_allreduce(self._h, C.c_void_p(int(device_ptr)), int(n_pixels)))

    def close(self):
        if self._h:
            lib().trhip_shutdown(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """A plain HIP device allocation for the *_device entry points, for hosts that do not hold a torch tensor: hipMalloc / hipMemcpy / hipFree of the HIP runtime
    libtracehip.so is linked against.  `ptr` is the device address."""
    _hip = None

    @classmethod
    def _rt(cls):
        if cls._hip is None:
            lib()  # libtracehip.so has loaded the runtime: open that very copy
            path = "libamdhip64.so"
            with open("/proc/self/maps") as maps:
                for line in maps:
                    if "libamdhip64.so" in line:
                        path = line.split()[-1]
                        break
            h = C.CDLL(path)
            h.hipMalloc.argtypes, h.hipMalloc.restype = [C.POINTER(_VP), C.c_size_t], C.c_int
            h.hipFree.argtypes, h.hipFree.restype = [_VP], C.c_int
            h.hipMemcpy.argtypes, h.hipMemcpy.restype = [_VP, _VP, C.c_size_t, C.c_int], C.c_int
            h.hipMemset.argtypes, h.hipMemset.restype = [_VP, C.c_int, C.c_size_t], C.c_int
            cls._hip = h
        return cls._hip

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = _VP()
        rc = self._rt().hipMalloc(C.byref(p), max(self.nbytes, 16))
        if rc:
            raise TraceHipError(f"hipMalloc of {self.nbytes} bytes failed ({rc})")
        self.ptr = p.value

    def zero(self):
        if self._rt().hipMemset(self.ptr, 0, self.nbytes):
            raise TraceHipError("hipMemset failed")
        return self

    def from_host(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        if a.nbytes != self.nbytes:
            raise TraceHipError(f"{a.nbytes} bytes given to a {self.nbytes}-byte device buffer")
        rc = self._rt().hipMemcpy(self.ptr, a.ctypes.data_as(_VP), self.nbytes, 1)  # hipMemcpyHostToDevice (blocking)
        if rc:
            raise TraceHipError(f"hipMemcpy failed ({rc})")
        return self

    def to_host(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        if out.nbytes != self.nbytes:
            raise TraceHipError(f"{out.nbytes} bytes asked of a {self.nbytes}-byte device buffer")
        rc = self._rt().hipMemcpy(out.ctypes.data_as(_VP), self.ptr, self.nbytes, 2)  # hipMemcpyDeviceToHost (blocking)
        if rc:
            raise TraceHipError(f"hipMemcpy failed ({rc})")
        return out

    def free(self):
        if getattr(self, "ptr", None):
            self._rt().hipFree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        dev = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("TRHIP_USE_LOCAL_RANK", "1") == "1" else 0
        _default_ctx = Context(dev)
    return _default_ctx
