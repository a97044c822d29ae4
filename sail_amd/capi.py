"""ctypes binding of libsail_hip.so (include/sail_hip.h) for the Python side (tests, bench).

The product host API is the JavaScript one in sail_amd/js (Sail.Renderer / Scene / Camera over the
N-API addon); this module is the same C ABI seen from Python. It never falls back to anything: if
the HIP library is missing or a call fails, it raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAIL_HIP_LIB: another build of the same library (a study variant, tools/study_build.sh), for the profiling tools
_PRODUCT_LIB = os.path.join(_HERE, "lib", "libsail_hip.so")
LIB_PATH = os.environ.get("SAIL_HIP_LIB") or _PRODUCT_LIB

SAIL_OK = 0
FLAG_AOV = 1
FLAG_SEGMENT_COUNT = 2
ACCUM_SUM, ACCUM_MIX, ACCUM_COMPAT8 = 0, 1, 2
PART_TILES, PART_SAMPLES = 0, 1
FILTER_COLOR, FILTER_GAMMA, FILTER_TONEMAPPING, FILTER_WINDOW = 0, 1, 2, 3
FILTER_WAVELET, FILTER_NORMAL, FILTER_POSITION = 4, 5, 6  # need FLAG_AOV
# sail_set_debug options (test / study switches; none changes a result)
DEBUG_CULL_MIN_PRIMS, DEBUG_FORCE_GENERIC, DEBUG_CULL_FMA, DEBUG_SAMPLE_GROUPS, DEBUG_FORCE_RCCL = 1, 2, 3, 4, 5
DEBUG_WAVEFRONT = 6
DEBUG_GROUP_ROUNDS = 7
DEBUG_CULL_GROUP_ROUNDS = 8
DEBUG_JIT = 9
JIT_NO_ROWDEFER = 64  # DEBUG_JIT bit, inverted: the value kernel without its deferred Sphere row (include/sail_hip.h)
DEBUG_JIT_WAIT = 10  # ms a launch waits for the scene's run-time kernel (-1: until built; the C ABI's default is 0)
DEBUG_JIT_NT = 12  # threads per workgroup of the run-time kernels (0: the form's own)
DEBUG_JIT_NS = 11  # samples of each pixel in flight per workgroup of the run-time kernels (0: the form's default)
DEBUG_JIT_VALUES_AFTER = 13  # samples at rest before the kernel compiled for the rows' values is asked for (0: at once, < 0: never)
KERNEL_JIT_NONE, KERNEL_JIT_PENDING, KERNEL_JIT_READY, KERNEL_JIT_FAILED = 0, 1, 2, 3
JIT_MODE_FLAT, JIT_MODE_CULL, JIT_MODE_ROOM = 0, 1, 2  # sail_jit_compile kernel forms (include/sail_hip.h)
# applied to every Context at creation (tests set entries with monkeypatch.setitem)
DEBUG_DEFAULTS: dict = {}

# exported symbols (kept in sync with include/sail_hip.h; tests/test_capi_symbols.py checks both ways)
EXPORTS = (
    "sail_create", "sail_create_multi", "sail_set_debug", "sail_destroy", "sail_last_error", "sail_device_count", "sail_device_info", "sail_set_scene",
    "sail_update_objects", "sail_set_accum_mode", "sail_set_partition", "sail_set_launch_samples",
    "sail_render", "sail_render_schedule", "sail_reset", "sail_sync", "sail_readback", "sail_read_accum",
    "sail_filter", "sail_get_stats", "sail_camera", "sail_jitter_inverse", "sail_schedule",
    "sail_comm_unique_id", "sail_comm_init", "sail_reduce", "sail_accum_device_ptr", "sail_partition_tiles",
    "sail_prim_bounds", "sail_math_probe", "sail_pick", "sail_kernel_name", "sail_filter_ms",
    "sail_abi_version", "sail_accum_parts", "sail_save_accum", "sail_load_accum", "sail_jit_compile",
    "sail_get_kernel_info", "sail_kernel_ready", "sail_set_jit_cache", "sail_jit_prebuild",
    "sail_jit_value_key", "sail_jit_spec_key", "sail_plan_settle", "sail_jit_resident",
    "sail_plan_reduce", "sail_plan_keep", "sail_plan_load_part", "sail_plan_last_bounce", "sail_plan_launch",
    "sail_noise_mark", "sail_noise_estimate", "sail_plan_until", "sail_render_until",
    "sail_set_active_tiles", "sail_get_active_tiles", "sail_plan_adaptive", "sail_adaptive_defaults", "sail_render_adaptive",
    "sail_denoise_defaults", "sail_denoise",
    "sail_temporal_defaults", "sail_gbuffer", "sail_temporal_begin", "sail_temporal_resolve", "sail_temporal_read",
    "sail_temporal_load_history",
    "sail_temporal_moments", "sail_temporal_load_moments", "sail_temporal_read_moments",
    "sail_temporal_filter_defaults", "sail_temporal_filter",
    "sail_move_objects", "sail_temporal_pending_motion",
    "sail_albedo", "sail_albedo_load", "sail_albedo_read", "sail_denoise_albedo", "sail_temporal_filter_albedo",
    "sail_guides", "sail_guides_load", "sail_guides_read", "sail_use_guides",
)


class SailError(RuntimeError):
    pass


class Plugins(ctypes.Structure):
    _fields_ = [("shape_mask", ctypes.c_uint32), ("material_mask", ctypes.c_uint32),
                ("texture_mask", ctypes.c_uint32), ("light_mask", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_uint64), ("segments", ctypes.c_uint64),
                ("nominal_segments", ctypes.c_uint64), ("kernel_ms", ctypes.c_double),
                ("last_launch_ms", ctypes.c_double), ("launches", ctypes.c_uint32)]


class KernelInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("build_id", ctypes.c_uint64), ("jit_state", ctypes.c_int),
                ("jit_from_cache", ctypes.c_int), ("jit_compile_ms", ctypes.c_double), ("jit_build_id", ctypes.c_uint64),
                ("jit_error", ctypes.c_char * 256)]


class ReducePlan(ctypes.Structure):
    _fields_ = [("receives", ctypes.c_int), ("tiles", ctypes.c_int), ("aov_owner", ctypes.c_int),
                ("send_own_aovs", ctypes.c_int), ("samples", ctypes.c_uint64)]


LAUNCH_TIER_NONE, LAUNCH_TIER_TYPES, LAUNCH_TIER_VALUE = 0, 1, 2  # sail_plan_launch: the tier a context has loaded


class LaunchFacts(ctypes.Structure):
    _fields_ = [("objects", ctypes.POINTER(ctypes.c_float)), ("texparams", ctypes.POINTER(ctypes.c_float)),
                ("plugins", ctypes.POINTER(Plugins)), ("n", ctypes.c_int), ("tn", ctypes.c_int), ("ln", ctypes.c_int),
                ("debug_set", ctypes.c_uint32), ("debug", ctypes.c_int * 16), ("launch_spp", ctypes.c_int),
                ("width", ctypes.c_int), ("height", ctypes.c_int), ("rank", ctypes.c_int), ("world", ctypes.c_int),
                ("part_mode", ctypes.c_int), ("compute_units", ctypes.c_int),
                ("nspp", ctypes.c_int), ("active_tiles", ctypes.c_int), ("cull_fma_ok", ctypes.c_int),
                ("eye_near_scene", ctypes.c_int), ("tier", ctypes.c_int)]


class LaunchPlan(ctypes.Structure):
    _fields_ = [("kernel_set", ctypes.c_int), ("cull_prims", ctypes.c_int), ("cull_primary", ctypes.c_int),
                ("wavefront", ctypes.c_int), ("jit_mode", ctypes.c_int), ("ns", ctypes.c_int),
                ("sample_groups", ctypes.c_int), ("group_spp", ctypes.c_int), ("group_home", ctypes.c_int),
                ("staged", ctypes.c_int), ("grid", ctypes.c_uint32), ("threads", ctypes.c_uint32),
                ("kernel_lights", ctypes.c_int), ("launch_samples", ctypes.c_int)]


class NoiseInfo(ctypes.Structure):
    _fields_ = [("mean", ctypes.c_double), ("max_tile", ctypes.c_double), ("k", ctypes.c_uint64), ("k_mark", ctypes.c_uint64),
                ("nonfinite", ctypes.c_uint64), ("tiles_x", ctypes.c_int), ("tiles_y", ctypes.c_int),
                ("kernel_ms", ctypes.c_double)]


class UntilStep(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint64), ("mean", ctypes.c_double), ("max_tile", ctypes.c_double)]


class AdaptiveParams(ctypes.Structure):
    _fields_ = [("target", ctypes.c_double), ("min_spp", ctypes.c_uint64), ("max_spp", ctypes.c_uint64),
                ("dilate", ctypes.c_int)]


class AdaptiveInfo(ctypes.Structure):
    _fields_ = [("noise", NoiseInfo), ("converged", ctypes.c_int), ("active_tiles", ctypes.c_int),
                ("tiles_x", ctypes.c_int), ("tiles_y", ctypes.c_int), ("pixel_samples", ctypes.c_uint64),
                ("frame_pixel_samples", ctypes.c_uint64), ("kernel_ms", ctypes.c_double)]


class DenoiseParams(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int), ("sigma_l", ctypes.c_float), ("sigma_x", ctypes.c_float),
                ("display", ctypes.c_int), ("gamma_c", ctypes.c_float)]


class DenoiseInfo(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint64), ("k_mark", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64),
                ("iterations", ctypes.c_int), ("kernel_ms", ctypes.c_double), ("pass_ms", ctypes.c_double * 8)]


class TemporalParams(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_float), ("pos_tol", ctypes.c_float), ("display", ctypes.c_int), ("gamma_c", ctypes.c_float)]


class TemporalInfo(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint64), ("hit_pixels", ctypes.c_uint64), ("history_pixels", ctypes.c_uint64),
                ("nonfinite", ctypes.c_uint64), ("kernel_ms", ctypes.c_double), ("pass_ms", ctypes.c_double * 3)]


# sail_temporal_read's maps
TEMPORAL_G_CUR, TEMPORAL_G_PREV, TEMPORAL_HIST, TEMPORAL_R, TEMPORAL_OUT = 0, 1, 2, 3, 4
# sail_temporal_read_moments' maps
TEMPORAL_M_HIST, TEMPORAL_M_R, TEMPORAL_M_OUT = 0, 1, 2


class TfilterParams(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int), ("sigma_l", ctypes.c_float), ("sigma_x", ctypes.c_float),
                ("min_hist", ctypes.c_float), ("display", ctypes.c_int), ("gamma_c", ctypes.c_float)]


class TfilterInfo(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint64), ("temporal_pixels", ctypes.c_uint64), ("spatial_pixels", ctypes.c_uint64),
                ("nonfinite", ctypes.c_uint64), ("iterations", ctypes.c_int), ("kernel_ms", ctypes.c_double),
                ("pass_ms", ctypes.c_double * 8)]


class AlbedoInfo(ctypes.Structure):
    _fields_ = [("hit_pixels", ctypes.c_uint64), ("partial_pixels", ctypes.c_uint64), ("grid", ctypes.c_int),
                ("kernel_ms", ctypes.c_double)]


class GuidesInfo(ctypes.Structure):
    _fields_ = [("hit_pixels", ctypes.c_uint64), ("followed_pixels", ctypes.c_uint64),
                ("truncated_pixels", ctypes.c_uint64), ("depth", ctypes.c_int), ("max_depth", ctypes.c_int),
                ("kernel_ms", ctypes.c_double)]


GUIDE_N, GUIDE_X = 0, 1         # sail_guide_map
ALBEDO_AMIN_DEFAULT = 0.01      # SAIL_ALBEDO_AMIN_DEFAULT: a guard, not a tuned value


_SHAPES = {"cube": 1, "sphere": 2, "rectangle": 3, "cone": 4, "cylinder": 5, "disk": 6,
           "hyperboloid": 7, "paraboloid": 8, "cornellbox": 9}
_MATERIALS = {"matte": 1, "mirror": 2, "metal": 3, "glass": 4}
_TEXTURES = {"checkerboard": 5, "checkerboard2": 7, "bilerp": 8, "mixf": 9, "scale": 10, "uvf": 11}
_LIGHTS = {"area": 0, "point": 1, "spot": 2}


def plugin_masks(plugins: dict) -> tuple:
    """Scene.tracerConfig() plugin-name lists -> category bit masks (src/scene/scene.js:70-112)."""
    def mask(names, table):
        m = 0
        for nm in names:
            m |= 1 << table[nm]
        return m
    return (mask(plugins.get("shape", []), _SHAPES), mask(plugins.get("material", []), _MATERIALS),
            mask(plugins.get("texture", []), _TEXTURES), mask(plugins.get("light", []), _LIGHTS))


_lib = None


def load(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libsail_hip.so (raises if it is absent: there is no CPU fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise SailError(f"HIP library not built: {p} (run python -c 'import __graft_entry__ as g; g.build()')")
    lib = ctypes.CDLL(p)
    f32p = ctypes.POINTER(ctypes.c_float)
    f64p = ctypes.POINTER(ctypes.c_double)
    vp = ctypes.c_void_p
    sig = {
        "sail_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]),
        "sail_create_multi": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                             ctypes.c_int, ctypes.c_uint32]),
        "sail_set_debug": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        "sail_destroy": (None, [vp]),
        "sail_last_error": (ctypes.c_char_p, [vp]),
        "sail_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
        "sail_device_info": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
        "sail_set_scene": (ctypes.c_int, [vp, f32p, ctypes.c_int, f32p, ctypes.c_int, f32p, ctypes.c_int, ctypes.POINTER(Plugins)]),
        "sail_update_objects": (ctypes.c_int, [vp, f32p, ctypes.c_int]),
        "sail_set_accum_mode": (ctypes.c_int, [vp, ctypes.c_int]),
        "sail_set_partition": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        "sail_set_launch_samples": (ctypes.c_int, [vp, ctypes.c_int]),
        "sail_render": (ctypes.c_int, [vp, f32p, f32p, ctypes.c_float, ctypes.c_int]),
        "sail_render_schedule": (ctypes.c_int, [vp, f32p, f32p, f32p, ctypes.c_int, ctypes.c_int]),
        "sail_reset": (ctypes.c_int, [vp]),
        "sail_sync": (ctypes.c_int, [vp]),
        "sail_readback": (ctypes.c_int, [vp, f32p, f32p, f32p]),
        "sail_read_accum": (ctypes.c_int, [vp, f32p]),
        "sail_filter": (ctypes.c_int, [vp, ctypes.c_int, f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float, f32p, ctypes.POINTER(ctypes.c_uint8)]),
        "sail_get_stats": (ctypes.c_int, [vp, ctypes.POINTER(Stats)]),
        "sail_camera": (ctypes.c_int, [f64p, f64p, f64p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, f64p]),
        "sail_jitter_inverse": (ctypes.c_int, [f64p, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, f32p]),
        "sail_schedule": (ctypes.c_int, [f64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, f32p, f32p]),
        "sail_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
        "sail_comm_init": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]),
        "sail_reduce": (ctypes.c_int, [vp, ctypes.c_int]),
        "sail_accum_device_ptr": (ctypes.c_int, [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]),
        "sail_partition_tiles": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
        "sail_prim_bounds": (ctypes.c_int, [f32p, ctypes.c_int, ctypes.c_int, f32p]),
        "sail_plan_last_bounce": (ctypes.c_int, [f32p, ctypes.c_int, f32p, ctypes.c_int, ctypes.POINTER(Plugins), ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)]),
        "sail_math_probe": (ctypes.c_int, [ctypes.c_int, f32p, f32p, f32p, ctypes.c_int]),
        "sail_abi_version": (ctypes.c_int, []),
        "sail_pick": (ctypes.c_int, [vp, f32p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), f32p]),
        "sail_kernel_name": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_int]),
        "sail_filter_ms": (ctypes.c_int, [vp, f64p]),
        "sail_accum_parts": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int)]),
        "sail_save_accum": (ctypes.c_int, [vp, ctypes.c_int, f32p, ctypes.POINTER(ctypes.c_uint64)]),
        "sail_load_accum": (ctypes.c_int, [vp, ctypes.c_int, f32p, ctypes.c_uint64]),
        "sail_jit_compile": (ctypes.c_int, [ctypes.POINTER(Plugins), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                                            vp, ctypes.POINTER(ctypes.c_size_t)]),
        "sail_get_kernel_info": (ctypes.c_int, [vp, ctypes.POINTER(KernelInfo)]),
        "sail_kernel_ready": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "sail_set_jit_cache": (ctypes.c_int, [ctypes.c_char_p]),
        "sail_jit_prebuild": (ctypes.c_int, [f32p, ctypes.c_int, f32p, ctypes.c_int, f32p, ctypes.c_int, ctypes.POINTER(Plugins),
                                             ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
        "sail_jit_value_key": (ctypes.c_int, [f32p, ctypes.c_int, f32p, ctypes.c_int, ctypes.POINTER(Plugins), ctypes.c_char_p,
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]),
        "sail_jit_spec_key": (ctypes.c_int, [f32p, ctypes.c_int, f32p, ctypes.c_int, ctypes.POINTER(Plugins), ctypes.c_char_p,
                                             ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p,
                                             ctypes.POINTER(ctypes.c_size_t)]),
        "sail_plan_settle": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int]),
        "sail_plan_launch": (ctypes.c_int, [ctypes.POINTER(LaunchFacts), ctypes.POINTER(LaunchPlan)]),
        "sail_jit_resident": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
        "sail_plan_reduce": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ReducePlan)]),
        "sail_plan_keep": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, f32p, f32p]),
        "sail_plan_load_part": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                                               ctypes.c_int, ctypes.c_uint64]),
        "sail_noise_mark": (ctypes.c_int, [vp]),
        "sail_noise_estimate": (ctypes.c_int, [vp, ctypes.POINTER(NoiseInfo), f32p, f32p, ctypes.c_int]),
        "sail_plan_until": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "sail_set_active_tiles": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int]),
        "sail_get_active_tiles": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "sail_plan_adaptive": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, f32p, ctypes.c_double, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8), f64p,
                                              ctypes.POINTER(ctypes.c_int)]),
        "sail_adaptive_defaults": (ctypes.c_int, [ctypes.POINTER(AdaptiveParams)]),
        "sail_render_adaptive": (ctypes.c_int, [vp, f64p, f32p, ctypes.c_int, ctypes.POINTER(AdaptiveParams),
                                                ctypes.POINTER(AdaptiveInfo), ctypes.POINTER(UntilStep), ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]),
        "sail_render_until": (ctypes.c_int, [vp, f64p, f32p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.POINTER(NoiseInfo), ctypes.POINTER(ctypes.c_int),
                                             ctypes.POINTER(UntilStep), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "sail_denoise_defaults": (ctypes.c_int, [ctypes.POINTER(DenoiseParams)]),
        "sail_denoise": (ctypes.c_int, [vp, ctypes.POINTER(DenoiseParams), f32p, f32p, ctypes.POINTER(ctypes.c_uint8),
                                        ctypes.POINTER(DenoiseInfo)]),
        "sail_temporal_defaults": (ctypes.c_int, [ctypes.POINTER(TemporalParams)]),
        "sail_gbuffer": (ctypes.c_int, [vp, f64p, f32p, f32p, ctypes.POINTER(ctypes.c_int32), f32p, f32p]),
        "sail_temporal_begin": (ctypes.c_int, [vp, f64p, f32p, ctypes.POINTER(TemporalParams), ctypes.POINTER(TemporalInfo)]),
        "sail_temporal_resolve": (ctypes.c_int, [vp, ctypes.POINTER(TemporalParams), f32p, ctypes.POINTER(ctypes.c_uint8),
                                                 ctypes.POINTER(TemporalInfo)]),
        "sail_temporal_read": (ctypes.c_int, [vp, ctypes.c_int, f32p]),
        "sail_temporal_load_history": (ctypes.c_int, [vp, f32p, f32p, f64p, f32p]),
        "sail_temporal_moments": (ctypes.c_int, [vp, ctypes.c_int]),
        "sail_temporal_load_moments": (ctypes.c_int, [vp, f32p]),
        "sail_temporal_read_moments": (ctypes.c_int, [vp, ctypes.c_int, f32p]),
        "sail_temporal_filter_defaults": (ctypes.c_int, [ctypes.POINTER(TfilterParams)]),
        "sail_temporal_filter": (ctypes.c_int, [vp, ctypes.POINTER(TfilterParams), f32p, f32p,
                                                ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(TfilterInfo)]),
        "sail_move_objects": (ctypes.c_int, [vp, f32p, ctypes.c_int, f32p, ctypes.c_float]),
        "sail_temporal_pending_motion": (ctypes.c_int, [vp, f32p, f32p, ctypes.POINTER(ctypes.c_int)]),
        "sail_albedo": (ctypes.c_int, [vp, f64p, f32p, ctypes.c_int, f32p, ctypes.POINTER(AlbedoInfo)]),
        "sail_albedo_load": (ctypes.c_int, [vp, f32p, f64p, f32p]),
        "sail_albedo_read": (ctypes.c_int, [vp, f32p]),
        "sail_guides": (ctypes.c_int, [vp, f64p, f32p, ctypes.c_int, f32p, f32p, ctypes.POINTER(GuidesInfo)]),
        "sail_guides_load": (ctypes.c_int, [vp, f32p, f32p, f64p, f32p]),
        "sail_guides_read": (ctypes.c_int, [vp, ctypes.c_int, f32p]),
        "sail_use_guides": (ctypes.c_int, [vp, ctypes.c_int]),
        "sail_denoise_albedo": (ctypes.c_int, [vp, ctypes.POINTER(DenoiseParams), ctypes.c_float, f32p, f32p,
                                               ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(DenoiseInfo)]),
        "sail_temporal_filter_albedo": (ctypes.c_int, [vp, ctypes.POINTER(TfilterParams), ctypes.c_float, f32p, f32p,
                                                       ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(TfilterInfo)]),
    }
    for name, (res, args) in sig.items():
        # another build (a path, or SAIL_HIP_LIB: tools/rev_build.sh builds older revisions as A/B controls) may predate
        # an entry point; the product's own library must have them all
        fn = getattr(lib, name) if p == _PRODUCT_LIB else getattr(lib, name, None)
        if fn is None:
            continue
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _ptr(a: Optional[np.ndarray], ct=ctypes.c_float):
    if a is None:
        return ctypes.cast(None, ctypes.POINTER(ct))
    return a.ctypes.data_as(ctypes.POINTER(ct))


# ---- host math (no device needed) ----------------------------------------------------------------------
def camera(eye, center, up=(0.0, 1.0, 0.0), fovy=55.0, aspect=1.0, znear=1.0, zfar=100.0) -> np.ndarray:
    lib = load()
    e, c, u = (np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in (eye, center, up))
    out = np.zeros(16, dtype=np.float64)
    rc = lib.sail_camera(_ptr(e, ctypes.c_double), _ptr(c, ctypes.c_double), _ptr(u, ctypes.c_double),
                         fovy, aspect, znear, zfar, _ptr(out, ctypes.c_double))
    if rc:
        raise SailError(f"sail_camera: {rc}")
    return out.reshape(4, 4)


def jitter_inverse(mvp: np.ndarray, jx: float, jy: float, width: int, height: int) -> np.ndarray:
    lib = load()
    m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
    out = np.zeros(16, dtype=np.float32)
    rc = lib.sail_jitter_inverse(_ptr(m, ctypes.c_double), jx, jy, width, height, _ptr(out))
    if rc:
        raise SailError(f"sail_jitter_inverse: {rc}")
    return out


def schedule(mvp: np.ndarray, width: int, height: int, k0: int, spp: int):
    """The frozen sample schedule: (spp x 16 f32 inverse matrices, spp f32 seeds)."""
    lib = load()
    m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
    inv = np.zeros((spp, 16), dtype=np.float32)
    seeds = np.zeros(spp, dtype=np.float32)
    rc = lib.sail_schedule(_ptr(m, ctypes.c_double), width, height, k0, spp, _ptr(inv), _ptr(seeds))
    if rc:
        raise SailError(f"sail_schedule: {rc}")
    return inv, seeds


def partition_tiles(width: int, height: int, rank: int, world: int) -> np.ndarray:
    """(x0, y0, w, h) of the 64x64 tiles a rank owns (tile t -> rank t % world)."""
    lib = load()
    n = lib.sail_partition_tiles(width, height, rank, world, ctypes.cast(None, ctypes.POINTER(ctypes.c_int)), 0)
    if n < 0:
        raise SailError(f"sail_partition_tiles: {n}")
    out = np.zeros((max(n, 1), 4), dtype=np.int32)
    lib.sail_partition_tiles(width, height, rank, world, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n)
    return out[:n]


def plan_reduce(width: int, height: int, rank: int, world: int, mode: int, k: int, root: int = 0) -> dict:
    """The library's reduce bookkeeping for one rank (sail_plan_reduce, host-only): receives, tiles, aov_owner,
    send_own_aovs, samples."""
    lib = load()
    p = ReducePlan()
    rc = lib.sail_plan_reduce(width, height, rank, world, mode, k, root, ctypes.byref(p))
    if rc:
        raise SailError(f"sail_plan_reduce: {rc}: {lib.sail_last_error(None).decode()}")
    return {f: getattr(p, f) for f, _ in ReducePlan._fields_}


def plan_keep(width: int, height: int, rank: int, world: int, mode: int, sums: np.ndarray) -> np.ndarray:
    """What a rank keeps of a whole-frame accumulator when resuming from it (sail_plan_keep, host-only)."""
    lib = load()
    src = _f32(sums).reshape(-1)
    if src.size != width * height * 4:
        raise SailError("plan_keep: sums must hold W*H*4 floats")
    out = np.empty_like(src)
    rc = lib.sail_plan_keep(width, height, rank, world, mode, _ptr(src), _ptr(out))
    if rc:
        raise SailError(f"sail_plan_keep: {rc}")
    return out.reshape(height, width, 4)


class LoadParts:
    """A part-wise checkpoint load's bookkeeping (sail_plan_load_part, host-only): the parts still missing and the
    checkpoint's sample index."""

    def __init__(self, parts: int):
        self.parts = parts
        self.missing = ctypes.c_uint64(0)
        self.k = ctypes.c_uint64(0)

    def load(self, part: int, k: int) -> None:
        lib = load()
        rc = lib.sail_plan_load_part(ctypes.byref(self.missing), ctypes.byref(self.k), self.parts, part, k)
        if rc:
            raise SailError(lib.sail_last_error(None).decode())

    @property
    def complete(self) -> bool:
        return self.missing.value == 0


def plan_until(k: int, min_spp: int, max_spp: int) -> int:
    """The next look of render_until's doubling schedule after k samples (sail_plan_until, host-only): min_spp first,
    then 2k capped at max_spp; k itself once max_spp is reached."""
    lib = load()
    for v in (k, min_spp, max_spp):
        if not 0 <= int(v) < 1 << 64:
            raise SailError(f"plan_until: {v} is not an unsigned 64-bit count")
    nxt = ctypes.c_uint64(0)
    rc = lib.sail_plan_until(int(k), int(min_spp), int(max_spp), ctypes.byref(nxt))
    if rc:
        raise SailError(f"sail_plan_until: {rc}: {lib.sail_last_error(None).decode()}")
    return int(nxt.value)


def plan_adaptive(width: int, height: int, tile_err16, target: float, dilate: int = 1, prev_active=None):
    """The next tile mask from a noise estimate's "tile_err" map (sail_plan_adaptive, host-only): per 64x64 tile the
    pixel-weighted mean e64 of its 16x16 tiles' errors; a tile stays active while it was active and it, or with dilate one
    of its neighbours, is not <= target. Returns (active (tilesY, tilesX) uint8, e64 (tilesY, tilesX) f64, n_active)."""
    lib = load()
    tx, ty = (int(width) + 63) // 64, (int(height) + 63) // 64
    e16 = _f32(tile_err16)
    if width < 1 or height < 1 or e16.size != ((int(width) + 15) // 16) * ((int(height) + 15) // 16):
        raise SailError(f"plan_adaptive: tile_err16 has {e16.size} entries for {width} x {height}")
    prev = None
    if prev_active is not None:
        prev = np.ascontiguousarray(np.asarray(prev_active, dtype=np.uint8).reshape(-1))
        if prev.size != tx * ty:
            raise SailError(f"plan_adaptive: prev_active has {prev.size} entries, the frame {tx * ty} tiles")
    active = np.zeros((ty, tx), dtype=np.uint8)
    e64 = np.zeros((ty, tx), dtype=np.float64)
    n = ctypes.c_int(0)
    rc = lib.sail_plan_adaptive(int(width), int(height), _ptr(e16), float(target), int(dilate), _ptr(prev, ctypes.c_uint8),
                                _ptr(active, ctypes.c_uint8), _ptr(e64, ctypes.c_double), ctypes.byref(n))
    if rc:
        raise SailError(f"sail_plan_adaptive: {rc}: {lib.sail_last_error(None).decode()}")
    return active, e64, int(n.value)


def adaptive_defaults() -> dict:
    """sail_render_adaptive's default parameters (sail_adaptive_defaults, host-only): target, min_spp, max_spp, dilate."""
    lib = load()
    p = AdaptiveParams()
    rc = lib.sail_adaptive_defaults(ctypes.byref(p))
    if rc:
        raise SailError(f"sail_adaptive_defaults: {rc}")
    return {"target": p.target, "min_spp": int(p.min_spp), "max_spp": int(p.max_spp), "dilate": p.dilate}


def _noise_dict(n: NoiseInfo) -> dict:
    return {"mean": n.mean, "max_tile": n.max_tile, "k": int(n.k), "k_mark": int(n.k_mark), "nonfinite": int(n.nonfinite),
            "tiles_x": n.tiles_x, "tiles_y": n.tiles_y, "kernel_ms": n.kernel_ms}


def denoise_defaults() -> dict:
    """sail_denoise's default parameters (sail_denoise_defaults, host-only): iterations, sigma_l, sigma_x, display,
    gamma_c."""
    lib = load()
    p = DenoiseParams()
    rc = lib.sail_denoise_defaults(ctypes.byref(p))
    if rc:
        raise SailError(f"sail_denoise_defaults: {rc}")
    return {"iterations": p.iterations, "sigma_l": p.sigma_l, "sigma_x": p.sigma_x, "display": p.display,
            "gamma_c": p.gamma_c}


def temporal_defaults() -> dict:
    """The temporal resolve's default parameters (sail_temporal_defaults, host-only): cap, pos_tol, display, gamma_c."""
    lib = load()
    p = TemporalParams()
    rc = lib.sail_temporal_defaults(ctypes.byref(p))
    if rc:
        raise SailError(f"sail_temporal_defaults: {rc}")
    return {"cap": p.cap, "pos_tol": p.pos_tol, "display": p.display, "gamma_c": p.gamma_c}


def temporal_filter_defaults() -> dict:
    """sail_temporal_filter's default parameters (sail_temporal_filter_defaults, host-only): iterations, sigma_l, sigma_x,
    min_hist, display, gamma_c."""
    lib = load()
    p = TfilterParams()
    rc = lib.sail_temporal_filter_defaults(ctypes.byref(p))
    if rc:
        raise SailError(f"sail_temporal_filter_defaults: {rc}")
    return {"iterations": p.iterations, "sigma_l": p.sigma_l, "sigma_x": p.sigma_x, "min_hist": p.min_hist,
            "display": p.display, "gamma_c": p.gamma_c}


def _temporal_params(params: Optional[dict], who: str):
    if params is None:
        return None
    d = temporal_defaults()
    unknown = set(params) - set(d)
    if unknown:
        raise SailError(f"{who}: unknown parameters {sorted(unknown)}")
    d.update(params)
    return TemporalParams(float(d["cap"]), float(d["pos_tol"]), int(d["display"]), float(d["gamma_c"]))


def _temporal_dict(i: TemporalInfo) -> dict:
    return {"k": int(i.k), "hit_pixels": int(i.hit_pixels), "history_pixels": int(i.history_pixels),
            "nonfinite": int(i.nonfinite), "kernel_ms": i.kernel_ms, "pass_ms": [i.pass_ms[j] for j in range(3)]}


def prim_bounds(objects, n: int, tn: int) -> np.ndarray:
    """Object3D.boundbox() answered by the pre-cull's padded bounds: (n, 2, 3) min / max per object row
    (host-only, no device)."""
    lib = load()
    rows = _f32(objects).reshape(-1)
    if rows.size < 18 * n:
        raise SailError("prim_bounds: fewer than 18 floats per row")
    out = np.zeros((max(n, 1), 6), dtype=np.float32)
    rc = lib.sail_prim_bounds(_ptr(rows), n, tn, _ptr(out))
    if rc:
        raise SailError(f"sail_prim_bounds: {rc}")
    return out[:n].reshape(n, 2, 3)


def plan_last_bounce(sc: dict, kernel_lights: bool):
    """(quiet row mask, skip_sort) of scene `sc` for a flat kernel with / without a light plugin compiled in
    (sail_plan_last_bounce, host-only): the rows whose hits add exactly +0 at a path's last bounce, and whether that
    bounce's path sort is skipped too."""
    lib = load()
    o, t = _f32(sc["objects"]), _f32(sc["texparams"])
    pl = Plugins(*[int(m) for m in plugin_masks(sc["plugins"])])
    quiet, skip = ctypes.c_uint32(0), ctypes.c_int(0)
    rc = lib.sail_plan_last_bounce(_ptr(o), sc["n"], _ptr(t), sc["tn"], ctypes.byref(pl), int(bool(kernel_lights)),
                                   ctypes.byref(quiet), ctypes.byref(skip))
    if rc:
        raise SailError(f"sail_plan_last_bounce: {rc}: {lib.sail_last_error(None).decode()}")
    return int(quiet.value), int(skip.value)


def math_probe(fn: int, x: np.ndarray, y: Optional[np.ndarray] = None) -> np.ndarray:
    lib = load()
    x = _f32(x)
    y = _f32(np.zeros_like(x) if y is None else y)
    out = np.zeros_like(x)
    rc = lib.sail_math_probe(fn, _ptr(x), _ptr(y), _ptr(out), int(x.size))
    if rc:
        raise SailError(f"sail_math_probe: {lib.sail_last_error(None).decode()}")
    return out


def device_count() -> int:
    lib = load()
    n = ctypes.c_int(0)
    lib.sail_device_count(ctypes.byref(n))
    return n.value


def device_info(device: int = 0):
    """(compute units, peak engine clock in Hz) of a device."""
    lib = load()
    cus, khz = ctypes.c_int(0), ctypes.c_int(0)
    if lib.sail_device_info(device, ctypes.byref(cus), ctypes.byref(khz)) != 0:
        raise SailError(f"sail_device_info({device}) failed")
    return cus.value, khz.value * 1e3


def set_jit_cache(path: Optional[str]):
    """The process-wide user cache of run-time code objects (None: the default under ~/.cache, "": none)."""
    load().sail_set_jit_cache(None if path is None else path.encode())


def jit_prebuild(sc: dict, arch: str = "gfx950", cache_dir: Optional[str] = None) -> bool:
    """Host-only: build the run-time kernel a default context derives for scene `sc` into `cache_dir` (default: the
    cache shipped beside the library, sail_amd/lib/jit). Returns whether the scene gets one."""
    lib = load()
    o, t, l = _f32(sc["objects"]), _f32(sc["texparams"]), _f32(sc["lights"])
    pl = Plugins(*[int(m) for m in plugin_masks(sc["plugins"])])
    built = ctypes.c_int(0)
    d = cache_dir or os.path.join(_HERE, "lib", "jit")
    rc = lib.sail_jit_prebuild(_ptr(o), sc["n"], _ptr(t), sc["tn"], _ptr(l), sc["ln"], ctypes.byref(pl), arch.encode(),
                               d.encode(), ctypes.byref(built))
    if rc:
        raise SailError(f"sail_jit_prebuild: {rc}: {lib.sail_last_error(None).decode()}")
    return bool(built.value)


def jit_value_key(sc: dict, arch: str = "gfx950", jit: Optional[int] = None, value: bool = True):
    """Host-only, nothing is compiled: (key, source prefix) of the value kernel a default context derives for scene `sc`
    once it has settled; its cache object is <cache dir>-values/<key>.co. (None, "") when the scene gets no value kernel.
    jit: the context's DEBUG_JIT switches instead of the defaults; value=False: the types kernel under the value kernel."""
    if jit is not None or not value:
        return _jit_spec_key(sc, arch, -1 if jit is None else jit, value)
    lib = load()
    o, t = _f32(sc["objects"]), _f32(sc["texparams"])
    pl = Plugins(*[int(m) for m in plugin_masks(sc["plugins"])])
    key, size = ctypes.c_uint64(0), ctypes.c_size_t(0)
    buf = None
    for _ in range(2):  # the size, then the text
        rc = lib.sail_jit_value_key(_ptr(o), sc["n"], _ptr(t), sc["tn"], ctypes.byref(pl), arch.encode(), ctypes.byref(key),
                                    buf, ctypes.byref(size))
        if rc:
            raise SailError(f"sail_jit_value_key: {rc}: {lib.sail_last_error(None).decode()}")
        if size.value == 0:
            return None, ""
        if buf is None:
            buf = ctypes.create_string_buffer(size.value)
    return f"{key.value:016x}", buf.value.decode()


def _jit_spec_key(sc: dict, arch: str, jit: int, value: bool):
    lib = load()
    o, t = _f32(sc["objects"]), _f32(sc["texparams"])
    pl = Plugins(*[int(m) for m in plugin_masks(sc["plugins"])])
    key, size = ctypes.c_uint64(0), ctypes.c_size_t(0)
    buf = None
    for _ in range(2):  # the size, then the text
        rc = lib.sail_jit_spec_key(_ptr(o), sc["n"], _ptr(t), sc["tn"], ctypes.byref(pl), arch.encode(), int(jit), int(value),
                                   ctypes.byref(key), buf, ctypes.byref(size))
        if rc:
            raise SailError(f"sail_jit_spec_key: {rc}: {lib.sail_last_error(None).decode()}")
        if size.value == 0:
            return None, ""
        if buf is None:
            buf = ctypes.create_string_buffer(size.value)
    return f"{key.value:016x}", buf.value.decode()


def jit_resident():
    """(code objects in host memory, modules loaded on devices) of value kernels in this process"""
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    load().sail_jit_resident(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def plan_settle(settled: int, after: int) -> bool:
    """Whether a context that rendered `settled` samples since its rows last changed asks for its value kernel under
    DEBUG_JIT_VALUES_AFTER = after"""
    return bool(load().sail_plan_settle(int(settled), int(after)))


def plan_launch(sc: dict, width: int, height: int, nspp: int, tier: int = LAUNCH_TIER_NONE, debug: Optional[dict] = None,
                launch_spp: int = 0, rank: int = 0, world: int = 1, part_mode: int = PART_TILES, compute_units: int = 256,
                active_tiles: int = -1, cull_fma_ok: bool = True, eye_near_scene: bool = True) -> dict:
    """Host-only (sail_plan_launch): the shape of one trace launch of `nspp` samples of scene `sc`, as a context with
    these facts derives it. debug: {DEBUG_* option: value} as given to a Context; tier: which run-time kernel the context
    has loaded (LAUNCH_TIER_*); active_tiles: the tiles a tile mask leaves of the rank's share (-1: no mask)."""
    lib = load()
    o, t = _f32(sc["objects"]), _f32(sc["texparams"])
    pl = Plugins(*[int(m) for m in plugin_masks(sc["plugins"])])
    f = LaunchFacts(objects=_ptr(o), texparams=_ptr(t), plugins=ctypes.pointer(pl), n=sc["n"], tn=sc["tn"], ln=sc["ln"],
                    launch_spp=launch_spp, width=width, height=height, rank=rank, world=world, part_mode=part_mode,
                    compute_units=compute_units, nspp=nspp, active_tiles=active_tiles, cull_fma_ok=int(bool(cull_fma_ok)),
                    eye_near_scene=int(bool(eye_near_scene)), tier=tier)
    for opt, val in (debug or {}).items():
        if not 0 <= int(opt) < 16:
            raise SailError(f"sail_plan_launch: no debug option {opt}")
        f.debug_set |= 1 << int(opt)
        f.debug[int(opt)] = int(val)
    out = LaunchPlan()
    rc = lib.sail_plan_launch(ctypes.byref(f), ctypes.byref(out))
    if rc:
        raise SailError(f"sail_plan_launch: {rc}: {lib.sail_last_error(None).decode()}")
    return {name: int(getattr(out, name)) for name, _ in LaunchPlan._fields_}


def comm_unique_id() -> bytes:
    lib = load()
    buf = ctypes.create_string_buffer(128)
    rc = lib.sail_comm_unique_id(buf)
    if rc:
        raise SailError(f"sail_comm_unique_id: {lib.sail_last_error(None).decode()}")
    return buf.raw


class Context:
    """A device context: the MI355X counterpart of Sail's Renderer/Tracer GPU state. With `devices` (a list of
    device ordinals) it is one multi-device context (sail_create_multi): the frame is split across them and
    reduced into device 0 on readback."""

    def __init__(self, width: int, height: int, device: int = -1, flags: int = 0, devices: Optional[Sequence[int]] = None,
                 debug: Optional[dict] = None):
        self.lib = load()
        self.W, self.H = int(width), int(height)
        h = ctypes.c_void_p()
        if devices is not None:
            dv = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            rc = self.lib.sail_create_multi(ctypes.byref(h), self.W, self.H, dv, len(devices), flags)
            what = "sail_create_multi"
        else:
            rc = self.lib.sail_create(ctypes.byref(h), self.W, self.H, device, flags)
            what = "sail_create"
        if rc:
            raise SailError(f"{what}: {rc}: {self.lib.sail_last_error(None).decode()}")
        self.h = h
        self._accum_mode = ACCUM_SUM          # the C ABI's default (sail_create)
        self._partition = (0, 1, PART_TILES)  # (rank, world, mode): checkpoints record and check these
        # the tests and bench.py want the scene's run-time kernel from the first launch (the C ABI's interactive default,
        # 0, launches the precompiled kernel until the background build is done; tests set 0 to render across the swap)
        for opt, val in {DEBUG_JIT_WAIT: -1, **DEBUG_DEFAULTS, **(debug or {})}.items():
            self.set_debug(opt, val)

    def set_debug(self, option: int, value: int):
        self._check(self.lib.sail_set_debug(self.h, int(option), int(value)), "sail_set_debug")

    def _check(self, rc: int, what: str):
        if rc:
            raise SailError(f"{what}: {rc}: {self.lib.sail_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.sail_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, objects, n: int, texparams, tn: int, lights, ln: int, masks: Sequence[int]):
        o, t, l = _f32(objects), _f32(texparams), _f32(lights)
        pl = Plugins(*[int(m) for m in masks])
        self._check(self.lib.sail_set_scene(self.h, _ptr(o), n, _ptr(t), tn, _ptr(l), ln, ctypes.byref(pl)),
                    "sail_set_scene")
        self._n = int(n)

    def set_scene_dict(self, sc: dict):
        self.set_scene(sc["objects"], sc["n"], sc["texparams"], sc["tn"], sc["lights"], sc["ln"],
                       plugin_masks(sc["plugins"]))

    def set_accum_mode(self, mode: int):
        self._check(self.lib.sail_set_accum_mode(self.h, mode), "sail_set_accum_mode")
        self._accum_mode = int(mode)

    def set_partition(self, rank: int, world: int, mode: int = PART_TILES):
        self._check(self.lib.sail_set_partition(self.h, rank, world, mode), "sail_set_partition")
        self._partition = (int(rank), int(world), int(mode))

    def set_launch_samples(self, spp: int):
        self._check(self.lib.sail_set_launch_samples(self.h, spp), "sail_set_launch_samples")

    def render_schedule(self, inv: np.ndarray, seeds: np.ndarray, eye, max_bounces: int):
        inv, seeds, e = _f32(inv), _f32(seeds), _f32(eye)
        self._check(self.lib.sail_render_schedule(self.h, _ptr(inv), _ptr(seeds), _ptr(e), int(seeds.size), max_bounces),
                    "sail_render_schedule")

    def render(self, inv: np.ndarray, eye, seed: float, max_bounces: int):
        inv, e = _f32(inv), _f32(eye)
        self._check(self.lib.sail_render(self.h, _ptr(inv), _ptr(e), float(seed), max_bounces), "sail_render")

    def reset(self):
        self._check(self.lib.sail_reset(self.h), "sail_reset")

    def sync(self):
        self._check(self.lib.sail_sync(self.h), "sail_sync")

    def readback(self, aov: bool = False):
        rgba = np.zeros((self.H, self.W, 4), dtype=np.float32)
        n = p = None
        if aov:
            n = np.zeros_like(rgba)
            p = np.zeros_like(rgba)
        self._check(self.lib.sail_readback(self.h, _ptr(rgba), _ptr(n), _ptr(p)), "sail_readback")
        return (rgba, n, p) if aov else rgba

    def read_accum(self) -> np.ndarray:
        rgba = np.zeros((self.H, self.W, 4), dtype=np.float32)
        self._check(self.lib.sail_read_accum(self.h, _ptr(rgba)), "sail_read_accum")
        return rgba

    def filter(self, kind: int, weights16=None, rx: float = 0.0, ry: float = 0.0, gamma_c: float = 2.2,
               want_u8: bool = False):
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        out8 = np.zeros((self.H, self.W, 4), dtype=np.uint8) if want_u8 else None
        w = _f32(weights16) if weights16 is not None else None
        self._check(self.lib.sail_filter(self.h, kind, _ptr(w), rx, ry, gamma_c, _ptr(out),
                                         _ptr(out8, ctypes.c_uint8)), "sail_filter")
        return (out, out8) if want_u8 else out

    def pick(self, rays) -> tuple:
        """rays: (count, 6) origin+direction -> (object row index or -1, distance) per ray"""
        r = _f32(rays).reshape(-1, 6)
        idx = np.zeros(len(r), dtype=np.int32)
        t = np.zeros(len(r), dtype=np.float32)
        self._check(self.lib.sail_pick(self.h, _ptr(r), len(r), _ptr(idx, ctypes.c_int32), _ptr(t)), "sail_pick")
        return idx, t

    def noise_mark(self):
        """Snapshot the shown accumulator as the noise estimate's mark (sail_noise_mark)."""
        self._check(self.lib.sail_noise_mark(self.h), "sail_noise_mark")

    def noise_estimate(self, tiles: bool = False, pixels: bool = False, remark: bool = False) -> dict:
        """The frame's noise against the mark (sail_noise_estimate): mean, max_tile, k, k_mark, nonfinite, tiles_x,
        tiles_y, kernel_ms; with `tiles` the (tiles_y, tiles_x) mean error per 16x16 tile as "tile_err", with `pixels` the
        (H, W) map as "pixel_err". remark: the mark becomes the current accumulator in the same pass."""
        n = NoiseInfo()
        tx, ty = (self.W + 15) // 16, (self.H + 15) // 16
        t = np.zeros((ty, tx), dtype=np.float32) if tiles else None
        p = np.zeros((self.H, self.W), dtype=np.float32) if pixels else None
        self._check(self.lib.sail_noise_estimate(self.h, ctypes.byref(n), _ptr(t), _ptr(p), int(bool(remark))),
                    "sail_noise_estimate")
        out = _noise_dict(n)
        if tiles:
            out["tile_err"] = t
        if pixels:
            out["pixel_err"] = p
        return out

    def render_until(self, mvp, eye, max_bounces: int, target: float, min_spp: int = 16, max_spp: int = 65536) -> dict:
        """Render the frozen schedule from the context's sample index until the noise estimate's mean is <= target or
        max_spp samples are in (sail_render_until). Returns the last estimate's fields plus "converged" and "history",
        a list of {k, mean, max_tile} per look (the first look only marks: its mean is inf)."""
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        for v in (min_spp, max_spp):
            if not 0 <= int(v) < 1 << 64:
                raise SailError(f"render_until: {v} is not an unsigned 64-bit count")
        n, conv, looks = NoiseInfo(), ctypes.c_int(0), ctypes.c_int(0)
        cap = 64  # looks double k: more cannot happen below 2^31 samples
        hist = (UntilStep * cap)()
        self._check(self.lib.sail_render_until(self.h, _ptr(m, ctypes.c_double), _ptr(e), int(max_bounces), float(target),
                                               int(min_spp), int(max_spp), ctypes.byref(n), ctypes.byref(conv), hist, cap,
                                               ctypes.byref(looks)), "sail_render_until")
        out = _noise_dict(n)
        out["converged"] = bool(conv.value)
        out["history"] = [{"k": int(s.k), "mean": s.mean, "max_tile": s.max_tile} for s in hist[:min(looks.value, cap)]]
        return out

    def set_active_tiles(self, active=None):
        """The mask over the frame's 64x64 tiles (sail_set_active_tiles): `active` holds one entry per tile, row 0 =
        bottom, nonzero = traced; None removes the mask."""
        if active is None:
            self._check(self.lib.sail_set_active_tiles(self.h, None, 0), "sail_set_active_tiles")
            return
        a = np.ascontiguousarray((np.asarray(active).reshape(-1) != 0).astype(np.uint8))
        self._check(self.lib.sail_set_active_tiles(self.h, _ptr(a, ctypes.c_uint8), int(a.size)), "sail_set_active_tiles")

    def get_active_tiles(self) -> np.ndarray:
        """The mask as a (tilesY, tilesX) uint8 array of 0 / 1 (all ones without a mask; sail_get_active_tiles)."""
        tx, ty = (self.W + 63) // 64, (self.H + 63) // 64
        a = np.zeros((ty, tx), dtype=np.uint8)
        n = ctypes.c_int(0)
        self._check(self.lib.sail_get_active_tiles(self.h, _ptr(a, ctypes.c_uint8), tx * ty, ctypes.byref(n)),
                    "sail_get_active_tiles")
        return a

    def render_adaptive(self, mvp, eye, max_bounces: int, target: Optional[float] = None, min_spp: Optional[int] = None,
                        max_spp: Optional[int] = None, dilate: Optional[int] = None) -> dict:
        """Render the frozen schedule, freezing the 64x64 tiles whose error is <= target at a look, until none is active
        or max_spp samples are in (sail_render_adaptive). Returns the last estimate's fields plus "converged",
        "active_tiles", "pixel_samples", "frame_pixel_samples", "trace_ms", "history" as render_until, and
        "tile_samples", the (tilesY, tilesX) uint32 sample count each tile holds. Unset parameters are
        adaptive_defaults()."""
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        d = adaptive_defaults()
        for key, v in (("target", target), ("min_spp", min_spp), ("max_spp", max_spp), ("dilate", dilate)):
            if v is not None:
                d[key] = v
        for v in (d["min_spp"], d["max_spp"]):
            if not 0 <= int(v) < 1 << 64:
                raise SailError(f"render_adaptive: {v} is not an unsigned 64-bit count")
        p = AdaptiveParams(float(d["target"]), int(d["min_spp"]), int(d["max_spp"]), int(d["dilate"]))
        info, looks = AdaptiveInfo(), ctypes.c_int(0)
        cap = 64  # looks double k: more cannot happen below 2^31 samples
        hist = (UntilStep * cap)()
        tx, ty = (self.W + 63) // 64, (self.H + 63) // 64
        ts = np.zeros((ty, tx), dtype=np.uint32)
        self._check(self.lib.sail_render_adaptive(self.h, _ptr(m, ctypes.c_double), _ptr(e), int(max_bounces), ctypes.byref(p),
                                                  ctypes.byref(info), hist, cap, ctypes.byref(looks),
                                                  _ptr(ts, ctypes.c_uint32)), "sail_render_adaptive")
        out = _noise_dict(info.noise)
        out.update(converged=bool(info.converged), active_tiles=info.active_tiles, tiles64_x=info.tiles_x,
                   tiles64_y=info.tiles_y, pixel_samples=int(info.pixel_samples),
                   frame_pixel_samples=int(info.frame_pixel_samples), trace_ms=info.kernel_ms, tile_samples=ts)
        out["history"] = [{"k": int(s.k), "mean": s.mean, "max_tile": s.max_tile} for s in hist[:min(looks.value, cap)]]
        return out

    def denoise(self, params: Optional[dict] = None, want_var: bool = False, want_u8: bool = False,
                albedo: Optional[float] = None) -> dict:
        """The variance-guided a-trous denoiser over the frame, the noise mark and the AOV maps (sail_denoise). `params`
        overrides entries of denoise_defaults(). Returns "rgba" (H, W, 4) f32, with want_var "var" (H, W) f32, with
        want_u8 "u8" (H, W, 4) uint8 (the display transform), and k, k_mark, nonfinite, iterations, kernel_ms and
        pass_ms (prepare, then each a-trous pass). With `albedo` = amin (ALBEDO_AMIN_DEFAULT) the frame is divided by the
        context's albedo map before the filter and multiplied by it afterwards (sail_denoise_albedo)."""
        p = None
        if params is not None:
            d = denoise_defaults()
            unknown = set(params) - set(d)
            if unknown:
                raise SailError(f"denoise: unknown parameters {sorted(unknown)}")
            d.update(params)
            p = DenoiseParams(int(d["iterations"]), float(d["sigma_l"]), float(d["sigma_x"]), int(d["display"]),
                              float(d["gamma_c"]))
        info = DenoiseInfo()
        rgba = np.zeros((self.H, self.W, 4), dtype=np.float32)
        var = np.zeros((self.H, self.W), dtype=np.float32) if want_var else None
        u8 = np.zeros((self.H, self.W, 4), dtype=np.uint8) if want_u8 else None
        pp = ctypes.byref(p) if p is not None else None
        if albedo is None:
            self._check(self.lib.sail_denoise(self.h, pp, _ptr(rgba), _ptr(var), _ptr(u8, ctypes.c_uint8),
                                              ctypes.byref(info)), "sail_denoise")
        else:
            self._check(self.lib.sail_denoise_albedo(self.h, pp, float(albedo), _ptr(rgba), _ptr(var),
                                                     _ptr(u8, ctypes.c_uint8), ctypes.byref(info)), "sail_denoise_albedo")
        out = {"rgba": rgba, "k": int(info.k), "k_mark": int(info.k_mark), "nonfinite": int(info.nonfinite),
               "iterations": info.iterations, "kernel_ms": info.kernel_ms,
               "pass_ms": [info.pass_ms[i] for i in range(info.iterations + 1)]}
        if want_var:
            out["var"] = var
        if want_u8:
            out["u8"] = u8
        return out

    def albedo(self, mvp, eye, grid: int = 2) -> dict:
        """The albedo map of a view (sail_albedo): the mean surface colour of the first hits of grid x grid sub-pixel
        rays per pixel, kept by the context for denoise(albedo=...) and temporal_filter(albedo=...). Returns "rgba"
        (H, W, 4) f32 (.w: the rays that hit; (1, 1, 1, 0) where none did), hit_pixels, partial_pixels, grid and
        kernel_ms."""
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        info = AlbedoInfo()
        self._check(self.lib.sail_albedo(self.h, _ptr(m, ctypes.c_double), _ptr(e), int(grid), _ptr(out),
                                         ctypes.byref(info)), "sail_albedo")
        return {"rgba": out, "hit_pixels": int(info.hit_pixels), "partial_pixels": int(info.partial_pixels),
                "grid": info.grid, "kernel_ms": info.kernel_ms}

    def albedo_load(self, amap, mvp, eye):
        """Install an albedo map (H, W, 4) f32 for the view (mvp, eye) (sail_albedo_load)."""
        a = _f32(amap)
        if a.shape != (self.H, self.W, 4):
            raise SailError(f"albedo_load: the map must have shape {(self.H, self.W, 4)}")
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        self._check(self.lib.sail_albedo_load(self.h, _ptr(a), _ptr(m, ctypes.c_double), _ptr(e)), "sail_albedo_load")

    def albedo_read(self) -> np.ndarray:
        """The context's albedo map as (H, W, 4) f32 (sail_albedo_read)."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        self._check(self.lib.sail_albedo_read(self.h, _ptr(out)), "sail_albedo_read")
        return out

    def guides(self, mvp, eye, depth: int = 4) -> dict:
        """The guide maps of a view (sail_guides): the normal and position of the first surface that scatters, reached
        through at most `depth` mirror or smooth-glass surfaces, kept by the context for the filters under
        use_guides(True). Returns "n" (H, W, 4) f32 (the normal AOV's encoding, .w: the depth walked), "x" (H, W, 4) f32
        (the position AOV's encoding, .w: the object row; a miss is (NaN, NaN, NaN, -1)), hit_pixels, followed_pixels,
        truncated_pixels, depth, max_depth and kernel_ms."""
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        n = np.zeros((self.H, self.W, 4), dtype=np.float32)
        x = np.zeros((self.H, self.W, 4), dtype=np.float32)
        info = GuidesInfo()
        self._check(self.lib.sail_guides(self.h, _ptr(m, ctypes.c_double), _ptr(e), int(depth), _ptr(n), _ptr(x),
                                         ctypes.byref(info)), "sail_guides")
        return {"n": n, "x": x, "hit_pixels": int(info.hit_pixels), "followed_pixels": int(info.followed_pixels),
                "truncated_pixels": int(info.truncated_pixels), "depth": info.depth, "max_depth": info.max_depth,
                "kernel_ms": info.kernel_ms}

    def guides_load(self, n_map, x_map, mvp, eye):
        """Install guide maps (H, W, 4) f32 each for the view (mvp, eye) (sail_guides_load)."""
        n, x = _f32(n_map), _f32(x_map)
        if n.shape != (self.H, self.W, 4) or x.shape != (self.H, self.W, 4):
            raise SailError(f"guides_load: both maps must have shape {(self.H, self.W, 4)}")
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        self._check(self.lib.sail_guides_load(self.h, _ptr(n), _ptr(x), _ptr(m, ctypes.c_double), _ptr(e)),
                    "sail_guides_load")

    def guides_read(self, which: int) -> np.ndarray:
        """One of the context's guide maps (GUIDE_N, GUIDE_X) as (H, W, 4) f32 (sail_guides_read)."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        self._check(self.lib.sail_guides_read(self.h, int(which), _ptr(out)), "sail_guides_read")
        return out

    def use_guides(self, on: bool = True):
        """The four filters read the guide maps in the AOVs' place (sail_use_guides); off by default."""
        self._check(self.lib.sail_use_guides(self.h, 1 if on else 0), "sail_use_guides")

    def gbuffer(self, mvp, eye, rays: bool = False) -> dict:
        """The G-buffer pass for a view (sail_gbuffer): "id" (H, W) int32 object row of the first hit or -1, "t" (H, W)
        its distance (1e5 on a miss), "xyz" (H, W, 3) its world position (0 on a miss), with `rays` "rays" (H, W, 6) the
        pixels' origin and direction. Changes no temporal state."""
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        r = np.zeros((self.H, self.W, 6), dtype=np.float32) if rays else None
        idx = np.zeros((self.H, self.W), dtype=np.int32)
        t = np.zeros((self.H, self.W), dtype=np.float32)
        xyz = np.zeros((self.H, self.W, 3), dtype=np.float32)
        self._check(self.lib.sail_gbuffer(self.h, _ptr(m, ctypes.c_double), _ptr(e), _ptr(r), _ptr(idx, ctypes.c_int32),
                                          _ptr(t), _ptr(xyz)), "sail_gbuffer")
        out = {"id": idx, "t": t, "xyz": xyz}
        if rays:
            out["rays"] = r
        return out

    def temporal_begin(self, mvp, eye, params: Optional[dict] = None) -> dict:
        """The camera is now at this view (sail_temporal_begin): commits the view that was current, computes the new
        view's G-buffer and reprojects the history into it. `params` overrides entries of temporal_defaults(). Returns
        k, hit_pixels, history_pixels, nonfinite, kernel_ms and pass_ms (G-buffer, reproject, resolve)."""
        m = np.ascontiguousarray(np.asarray(mvp, dtype=np.float64).reshape(16))
        e = _f32(eye)
        p = _temporal_params(params, "temporal_begin")
        info = TemporalInfo()
        self._check(self.lib.sail_temporal_begin(self.h, _ptr(m, ctypes.c_double), _ptr(e),
                                                 ctypes.byref(p) if p is not None else None, ctypes.byref(info)),
                    "sail_temporal_begin")
        return _temporal_dict(info)

    def temporal_resolve(self, params: Optional[dict] = None, want_u8: bool = False) -> dict:
        """Blend the reprojected history with the samples of the current view (sail_temporal_resolve). Returns "rgba"
        (H, W, 4) f32: the resolved colour and its effective sample count, with want_u8 "u8" (H, W, 4) uint8 (the
        display transform), and the fields of temporal_begin."""
        p = _temporal_params(params, "temporal_resolve")
        info = TemporalInfo()
        rgba = np.zeros((self.H, self.W, 4), dtype=np.float32)
        u8 = np.zeros((self.H, self.W, 4), dtype=np.uint8) if want_u8 else None
        self._check(self.lib.sail_temporal_resolve(self.h, ctypes.byref(p) if p is not None else None, _ptr(rgba),
                                                   _ptr(u8, ctypes.c_uint8), ctypes.byref(info)), "sail_temporal_resolve")
        out = _temporal_dict(info)
        out["rgba"] = rgba
        if want_u8:
            out["u8"] = u8
        return out

    def temporal_read(self, which: int) -> np.ndarray:
        """One of the five temporal maps (TEMPORAL_G_CUR .. TEMPORAL_OUT) as (H, W, 4) f32 (sail_temporal_read)."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        self._check(self.lib.sail_temporal_read(self.h, int(which), _ptr(out)), "sail_temporal_read")
        return out

    def temporal_load_history(self, hist, g, mvp_prev, eye_prev):
        """Install a history (H, W, 4: rgb mean, sample count), its G-buffer (H, W, 4: position, object row) and its
        view as the committed one (sail_temporal_load_history)."""
        h, gg = _f32(hist), _f32(g)
        if h.shape != (self.H, self.W, 4) or gg.shape != (self.H, self.W, 4):
            raise SailError(f"temporal_load_history: maps must have shape {(self.H, self.W, 4)}")
        m = np.ascontiguousarray(np.asarray(mvp_prev, dtype=np.float64).reshape(16))
        e = _f32(eye_prev)
        self._check(self.lib.sail_temporal_load_history(self.h, _ptr(h), _ptr(gg), _ptr(m, ctypes.c_double), _ptr(e)),
                    "sail_temporal_load_history")

    def update_objects(self, objects):
        """New object rows, the same number as the scene's (sail_update_objects): the accumulation restarts and the
        temporal state goes."""
        o = _f32(objects)
        if o.size % 18:
            raise SailError("update_objects: object rows have 18 floats each")
        self._check(self.lib.sail_update_objects(self.h, _ptr(o), o.size // 18), "sail_update_objects")

    def move_objects(self, objects, motion=None, hist_cap: float = 0.0):
        """New object rows that keep the temporal state (sail_move_objects). `motion` is (n, 3) f32, each row's
        translation since the rows the context holds now (None: no row moved); `hist_cap` 0 for none, else the count a
        history that crosses the move is clamped to. The next temporal_begin reprojects with the motion."""
        o = _f32(objects)
        if o.size % 18:
            raise SailError("move_objects: object rows have 18 floats each")
        n = o.size // 18
        m = None
        if motion is not None:
            m = _f32(motion)
            if m.size != n * 3:
                raise SailError(f"move_objects: motion must have shape {(n, 3)}")
        self._check(self.lib.sail_move_objects(self.h, _ptr(o), n, _ptr(m), float(hist_cap)), "sail_move_objects")

    def temporal_pending_motion(self) -> dict:
        """What is pending for the next temporal_begin (sail_temporal_pending_motion): "motion" (n, 3) f32 for the n rows
        of the scene set through this object, "hist_cap" (inf when none) and "pending"."""
        n = getattr(self, "_n", 0)
        motion = np.zeros((n, 3), dtype=np.float32)
        cap = ctypes.c_float()
        pending = ctypes.c_int()
        self._check(self.lib.sail_temporal_pending_motion(self.h, _ptr(motion) if n else _ptr(None), ctypes.byref(cap),
                                                          ctypes.byref(pending)), "sail_temporal_pending_motion")
        return {"motion": motion, "hist_cap": float(cap.value), "pending": int(pending.value)}

    def temporal_moments(self, on: bool = True):
        """Switch the tracking of the luminance moments on (three more maps, zeroed) or off (freed)
        (sail_temporal_moments)."""
        self._check(self.lib.sail_temporal_moments(self.h, int(on)), "sail_temporal_moments")

    def temporal_load_moments(self, mom):
        """Install moments (H, W, 4: mu1, mu2, mm, 0) as those of the committed history, right after
        temporal_load_history (sail_temporal_load_moments)."""
        m = _f32(mom)
        if m.shape != (self.H, self.W, 4):
            raise SailError(f"temporal_load_moments: the map must have shape {(self.H, self.W, 4)}")
        self._check(self.lib.sail_temporal_load_moments(self.h, _ptr(m)), "sail_temporal_load_moments")

    def temporal_read_moments(self, which: int) -> np.ndarray:
        """One of the three moment maps (TEMPORAL_M_HIST, TEMPORAL_M_R, TEMPORAL_M_OUT) as (H, W, 4) f32
        (sail_temporal_read_moments)."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        self._check(self.lib.sail_temporal_read_moments(self.h, int(which), _ptr(out)), "sail_temporal_read_moments")
        return out

    def temporal_filter(self, params: Optional[dict] = None, want_var: bool = False, want_u8: bool = False,
                        albedo: Optional[float] = None) -> dict:
        """The a-trous passes over the resolved picture of the current view, steered by the variance of the tracked
        moments (sail_temporal_filter). `params` overrides entries of temporal_filter_defaults(). Returns "rgba"
        (H, W, 4) f32, with want_var "var" (H, W) f32, with want_u8 "u8" (H, W, 4) uint8 (the display transform), and k,
        temporal_pixels, spatial_pixels, nonfinite, iterations, kernel_ms and pass_ms (prepare, then each a-trous pass).
        With `albedo` = amin the picture is filtered divided by the context's albedo map, which must belong to the
        current temporal view (sail_temporal_filter_albedo)."""
        p = None
        if params is not None:
            d = temporal_filter_defaults()
            unknown = set(params) - set(d)
            if unknown:
                raise SailError(f"temporal_filter: unknown parameters {sorted(unknown)}")
            d.update(params)
            p = TfilterParams(int(d["iterations"]), float(d["sigma_l"]), float(d["sigma_x"]), float(d["min_hist"]),
                              int(d["display"]), float(d["gamma_c"]))
        info = TfilterInfo()
        rgba = np.zeros((self.H, self.W, 4), dtype=np.float32)
        var = np.zeros((self.H, self.W), dtype=np.float32) if want_var else None
        u8 = np.zeros((self.H, self.W, 4), dtype=np.uint8) if want_u8 else None
        pp = ctypes.byref(p) if p is not None else None
        if albedo is None:
            self._check(self.lib.sail_temporal_filter(self.h, pp, _ptr(rgba), _ptr(var), _ptr(u8, ctypes.c_uint8),
                                                      ctypes.byref(info)), "sail_temporal_filter")
        else:
            self._check(self.lib.sail_temporal_filter_albedo(self.h, pp, float(albedo), _ptr(rgba), _ptr(var),
                                                             _ptr(u8, ctypes.c_uint8), ctypes.byref(info)),
                        "sail_temporal_filter_albedo")
        out = {"rgba": rgba, "k": int(info.k), "temporal_pixels": int(info.temporal_pixels),
               "spatial_pixels": int(info.spatial_pixels), "nonfinite": int(info.nonfinite),
               "iterations": info.iterations, "kernel_ms": info.kernel_ms,
               "pass_ms": [info.pass_ms[i] for i in range(info.iterations + 1)]}
        if want_var:
            out["var"] = var
        if want_u8:
            out["u8"] = u8
        return out

    def filter_ms(self) -> float:
        v = ctypes.c_double()
        self._check(self.lib.sail_filter_ms(self.h, ctypes.byref(v)), "sail_filter_ms")
        return v.value

    def kernel_name(self) -> str:
        buf = ctypes.create_string_buffer(64)
        self._check(self.lib.sail_kernel_name(self.h, buf, 64), "sail_kernel_name")
        return buf.value.decode()

    def kernel_info(self) -> dict:
        k = KernelInfo()
        self._check(self.lib.sail_get_kernel_info(self.h, ctypes.byref(k)), "sail_get_kernel_info")
        return {"name": k.name.decode(), "build_id": f"{k.build_id:016x}", "jit_state": k.jit_state,
                "jit_from_cache": k.jit_from_cache, "jit_compile_ms": k.jit_compile_ms,
                "jit_build_id": f"{k.jit_build_id:016x}", "jit_error": k.jit_error.decode()}

    def kernel_id(self) -> str:
        """the last launch's kernel and its build identity, "name@hex16" (profiles are matched to kernels by it)"""
        k = self.kernel_info()
        return f"{k['name']}@{k['build_id']}"

    def kernel_ready(self, timeout_ms: int = -1) -> bool:
        r = ctypes.c_int(0)
        self._check(self.lib.sail_kernel_ready(self.h, int(timeout_ms), ctypes.byref(r)), "sail_kernel_ready")
        return bool(r.value)

    def stats(self) -> Stats:
        s = Stats()
        self._check(self.lib.sail_get_stats(self.h, ctypes.byref(s)), "sail_get_stats")
        return s

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        self._check(self.lib.sail_comm_init(self.h, uid, nranks, rank), "sail_comm_init")

    def reduce(self, root: int = 0):
        self._check(self.lib.sail_reduce(self.h, root), "sail_reduce")

    def _parts(self) -> int:
        n = ctypes.c_int(0)
        self._check(self.lib.sail_accum_parts(self.h, ctypes.byref(n)), "sail_accum_parts")
        return n.value

    def save(self) -> dict:
        """Checkpoint of the progressive render: {"k": next sample index, "parts": [H x W x 4 f32 accumulator per
        device], and the context it belongs to: width, height, accum_mode, partition (rank, world, mode)}
        (sail_save_accum)"""
        parts, k = [], ctypes.c_uint64(0)
        for i in range(self._parts()):
            a = np.zeros((self.H, self.W, 4), dtype=np.float32)
            self._check(self.lib.sail_save_accum(self.h, i, _ptr(a), ctypes.byref(k)), "sail_save_accum")
            parts.append(a)
        return {"k": int(k.value), "parts": parts, "width": self.W, "height": self.H,
                "accum_mode": self._accum_mode, "partition": list(self._partition)}

    def load(self, ckpt: dict):
        """Resume from save()'s checkpoint (every part, into a context of the same size, accumulation mode, partition
        and device count), or from a whole-frame accumulator {"k": k, "frame": H x W x 4} (sail_load_accum part -1).
        A checkpoint that does not fit this context raises SailError before anything is copied."""
        def arr(a, what):
            a = _f32(a)
            if a.shape != (self.H, self.W, 4):
                raise SailError(f"Context.load: {what} has shape {a.shape}, this context needs {(self.H, self.W, 4)}")
            return a
        for key, mine in (("width", self.W), ("height", self.H), ("accum_mode", self._accum_mode)):
            if key in ckpt and int(ckpt[key]) != mine:
                raise SailError(f"Context.load: checkpoint {key} {ckpt[key]} differs from this context's {mine}")
        if "partition" in ckpt and tuple(int(v) for v in ckpt["partition"]) != self._partition:
            raise SailError(f"Context.load: checkpoint partition {tuple(ckpt['partition'])} differs from {self._partition}")
        if "frame" in ckpt:
            f = arr(ckpt["frame"], "frame")
            self._check(self.lib.sail_load_accum(self.h, -1, _ptr(f), int(ckpt["k"])), "sail_load_accum")
            return
        parts = [arr(a, f"part {i}") for i, a in enumerate(ckpt["parts"])]
        if len(parts) != self._parts():
            raise SailError(f"Context.load: checkpoint has {len(parts)} parts, this context {self._parts()}")
        for i, a in enumerate(parts):
            self._check(self.lib.sail_load_accum(self.h, i, _ptr(a), int(ckpt["k"])), "sail_load_accum")

    def accum_device_ptr(self):
        p = ctypes.c_void_p()
        b = ctypes.c_size_t()
        self._check(self.lib.sail_accum_device_ptr(self.h, ctypes.byref(p), ctypes.byref(b)), "sail_accum_device_ptr")
        return p.value, b.value
