"""MI355X-native ray tracer — Python view of the C-ABI in include/rt_api.h.

The product is the HIP library ``lib/librtamd.so`` (gfx950 kernels + host C++). This module only
binds its C entry points with ctypes for tests and the bench; it never computes a frame itself and
there is no CPU fallback: if the library is missing, importing the package raises.

torch is imported first on purpose: it loads the HIP runtime that the library then shares, so
device pointers and hipStream_t handles from torch tensors are valid in the library.
"""
from __future__ import annotations

import ctypes
import gzip
import os
from typing import Iterable, Optional, Sequence

import numpy as np

try:  # share torch's HIP runtime when torch is present
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is part of the image
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_LIBRARY (diagnostics: tools/asan_check.sh's sanitizer build of the same library) overrides the path
LIB_PATH = os.environ.get("RT_LIBRARY") or os.path.join(_HERE, "lib", "librtamd.so")
ASSETS = os.path.join(_HERE, "assets")

RT_OK, RT_E_INVALID, RT_E_OOM, RT_E_HIP, RT_E_RCCL, RT_E_UNSUPPORTED, RT_E_IO = 0, -1, -2, -3, -4, -5, -6
RT_HITGROUP_MODEL, RT_HITGROUP_SHADOW, RT_HITGROUP_PLANE = 0, 1, 2
RT_SHADE_REF, RT_SHADE_LAMBERT_SHADOW, RT_SHADE_PRIMARY = 0, 1, 2
RT_SCHED_PACKET, RT_SCHED_LANE = 0, 1
RT_TRIANGLE_TEST_MOLLER_TRUMBORE, RT_TRIANGLE_TEST_WATERTIGHT = 0, 1
RT_BALANCE_INFO_COUNT = 20
RT_TILE_PLAN_STATS = 18
TILE_PLAN_STAT_NAMES = ("nitems", "nsplit", "want_extra", "max_cost", "mean_cost", "threshold", "plans", "pays", "bad",
                        "first_bad_tile", "first_bad_word", "phase_load_ticks", "phase_budget_ticks",
                        "phase_place_ticks", "coherent", "refused", "refused_plans", "slots")
RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH, RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES = 0x04, 0x10
RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES = 0x20
STAT_NAMES = ("primary_rays", "shadow_rays", "aabb_tests", "tri_tests", "instance_entries",
              "stack_overflows", "pixels", "dispatches", "reflection_rays", "node_fetches", "tri_fetches",
              "instance_fetches")


class RtError(RuntimeError):
    """Non-zero rt_status (the reference's ThrowIfFailed, DXSampleHelper.h:16-22)."""

    def __init__(self, status: int, msg: str = ""):
        self.status = status
        super().__init__(f"{_status_name(status)}: {msg}" if msg else _status_name(status))


class rt_instance(ctypes.Structure):
    _fields_ = [("blas", ctypes.c_uint32), ("xform3x4_rowmajor", ctypes.c_float * 12),
                ("instance_id", ctypes.c_uint32), ("hit_group", ctypes.c_uint32)]


class rt_light(ctypes.Structure):
    _fields_ = [("color", ctypes.c_float * 3), ("position", ctypes.c_float * 3),
                ("intensity", ctypes.c_float)]


class rt_material(ctypes.Structure):
    _fields_ = [("albedo", ctypes.c_float * 3), ("roughness", ctypes.c_float),
                ("metallic", ctypes.c_float), ("reflectivity", ctypes.c_float)]


class rt_bvh_info(ctypes.Structure):
    _fields_ = [("prim_count", ctypes.c_uint32), ("node_count", ctypes.c_uint32),
                ("depth", ctypes.c_uint32), ("max_stack", ctypes.c_uint32),
                ("bounds_lo", ctypes.c_float * 3), ("bounds_hi", ctypes.c_float * 3),
                ("build_ms", ctypes.c_double)]


class rt_gbuffer(ctypes.Structure):
    """include/rt_api.h rt_gbuffer: the output planes of rt_dispatch_gbuffer (device pointers, None: not written)."""
    _fields_ = [("hits", ctypes.c_void_p), ("uv", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("object", ctypes.c_void_p)]


class rt_gbuffer_motion(ctypes.Structure):
    """include/rt_api.h rt_gbuffer_motion: rt_gbuffer's planes and the motion plane of rt_dispatch_gbuffer_motion."""
    _fields_ = [("hits", ctypes.c_void_p), ("uv", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("object", ctypes.c_void_p), ("motion", ctypes.c_void_p)]


class rt_ao_params(ctypes.Structure):
    """include/rt_api.h rt_ao_params: samples (1..64), seed, radius (the rays' tmax), tmin of rt_dispatch_ao."""
    _fields_ = [("samples", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("radius", ctypes.c_float),
                ("tmin", ctypes.c_float)]


class rt_shadow_params(ctypes.Structure):
    """include/rt_api.h rt_shadow_params: samples (1..64), seed, light_radius, tmin of rt_dispatch_shadow."""
    _fields_ = [("samples", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("light_radius", ctypes.c_float),
                ("tmin", ctypes.c_float)]


class rt_resolve_inputs(ctypes.Structure):
    """include/rt_api.h rt_resolve_inputs: the planes rt_shade_resolve reads (vis and ao may be None)."""
    _fields_ = [("hits", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("object", ctypes.c_void_p),
                ("vis", ctypes.c_void_p), ("vis_stride", ctypes.c_uint64), ("ao", ctypes.c_void_p)]


RT_MAX_MATERIALS = 32


class rt_material_table(ctypes.Structure):
    """include/rt_api.h rt_material_table: a host array of materials and the optional instance -> material map (a
    device array for rt_shade_resolve_pbr, a host array for rt_host_shade_resolve_pbr)."""
    _fields_ = [("materials", ctypes.POINTER(rt_material)), ("nmaterials", ctypes.c_uint32),
                ("instance_material", ctypes.c_void_p), ("ninstances", ctypes.c_uint32)]


class rt_resolve_pbr_inputs(ctypes.Structure):
    """include/rt_api.h rt_resolve_pbr_inputs: rt_resolve_inputs' fields and the reflection pass's radiance plane."""
    _fields_ = [("hits", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("object", ctypes.c_void_p),
                ("vis", ctypes.c_void_p), ("vis_stride", ctypes.c_uint64), ("ao", ctypes.c_void_p),
                ("refl", ctypes.c_void_p)]


class rt_reflection_params(ctypes.Structure):
    """include/rt_api.h rt_reflection_params: samples (1..64), seed, roughness, tmax, shadow_tmin of
    rt_dispatch_reflection."""
    _fields_ = [("samples", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("roughness", ctypes.c_float),
                ("tmax", ctypes.c_float), ("shadow_tmin", ctypes.c_float)]


RT_REFLECT_FRAME_RAY = 1
RT_REFLECT_SHADOW_MODELS = 2


class rt_reflection_pbr_params(ctypes.Structure):
    """include/rt_api.h rt_reflection_pbr_params: rt_reflection_params' fields and the RT_REFLECT_* flags of
    rt_dispatch_reflection_pbr."""
    _fields_ = [("samples", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("roughness", ctypes.c_float),
                ("tmax", ctypes.c_float), ("shadow_tmin", ctypes.c_float), ("flags", ctypes.c_uint32)]


RT_MAX_REFLECTION_BOUNCES = 18


class rt_reflection_chain_params(ctypes.Structure):
    """include/rt_api.h rt_reflection_chain_params: rt_reflection_pbr_params' fields and max_bounces
    (1..RT_MAX_REFLECTION_BOUNCES) of rt_dispatch_reflection_chain."""
    _fields_ = [("samples", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("roughness", ctypes.c_float),
                ("tmax", ctypes.c_float), ("shadow_tmin", ctypes.c_float), ("flags", ctypes.c_uint32),
                ("max_bounces", ctypes.c_uint32)]


class rt_indirect_params(ctypes.Structure):
    """include/rt_api.h rt_indirect_params: samples (1..64), seed, tmax, shadow_tmin and the flags
    (RT_REFLECT_SHADOW_MODELS only) of rt_dispatch_indirect."""
    _fields_ = [("samples", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("tmax", ctypes.c_float),
                ("shadow_tmin", ctypes.c_float), ("flags", ctypes.c_uint32)]


class rt_resolve_gi_inputs(ctypes.Structure):
    """include/rt_api.h rt_resolve_gi_inputs: rt_resolve_pbr_inputs' fields, the indirect pass's radiance plane and its
    scale."""
    _fields_ = [("hits", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("object", ctypes.c_void_p),
                ("vis", ctypes.c_void_p), ("vis_stride", ctypes.c_uint64), ("ao", ctypes.c_void_p),
                ("refl", ctypes.c_void_p), ("indirect", ctypes.c_void_p), ("indirect_scale", ctypes.c_float)]


class rt_reflection_planes(ctypes.Structure):
    """include/rt_api.h rt_reflection_planes: the planes rt_dispatch_reflection writes (hits may be None)."""
    _fields_ = [("radiance", ctypes.c_void_p), ("hits", ctypes.c_void_p)]


class rt_reflection_composite_params(ctypes.Structure):
    """include/rt_api.h rt_reflection_composite_params: strength and f0 of rt_reflection_composite, both in [0, 1]."""
    _fields_ = [("strength", ctypes.c_float), ("f0", ctypes.c_float)]


class rt_ao_temporal_params(ctypes.Structure):
    """include/rt_api.h rt_ao_temporal_params: max_history (1..1024), depth_tol, normal_cos of rt_ao_accumulate."""
    _fields_ = [("max_history", ctypes.c_uint32), ("depth_tol", ctypes.c_float), ("normal_cos", ctypes.c_float)]


class rt_ao_atrous_params(ctypes.Structure):
    """include/rt_api.h rt_ao_atrous_params: iterations (1..5), depth_tol, normal_cos of rt_ao_atrous."""
    _fields_ = [("iterations", ctypes.c_uint32), ("depth_tol", ctypes.c_float), ("normal_cos", ctypes.c_float)]


class rt_radiance_temporal_params(ctypes.Structure):
    """include/rt_api.h rt_radiance_temporal_params: rt_ao_temporal_params' fields, for rt_radiance_accumulate."""
    _fields_ = [("max_history", ctypes.c_uint32), ("depth_tol", ctypes.c_float), ("normal_cos", ctypes.c_float)]


class rt_radiance_atrous_params(ctypes.Structure):
    """include/rt_api.h rt_radiance_atrous_params: iterations (1..5), depth_tol, normal_cos, sigma_l (> 0) of
    rt_radiance_atrous."""
    _fields_ = [("iterations", ctypes.c_uint32), ("depth_tol", ctypes.c_float), ("normal_cos", ctypes.c_float),
                ("sigma_l", ctypes.c_float)]


class rt_reflection_motion_params(ctypes.Structure):
    """include/rt_api.h rt_reflection_motion_params: share (0..1), static_tol (pixels, >= 0), depth_tol, normal_cos of
    rt_reflection_motion."""
    _fields_ = [("share", ctypes.c_float), ("static_tol", ctypes.c_float), ("depth_tol", ctypes.c_float),
                ("normal_cos", ctypes.c_float)]


# rt_reflection_motion's static_tol default: 16 x the largest |e_s - m| measured on static geometry (0.00256 px on C2F
# at 1080p, 0.00049 px on REFLO at 720p, under an eye move of (0.3, 0.15, -0.2); tools/reflection_motion_study.py,
# DESIGN §3.19) = 0.041 px, rounded up to a power of two; the cap of 0.25 px is not reached.
REFLECTION_MOTION_STATIC_TOL = 2.0 ** -4


class rt_upscale_params(ctypes.Structure):
    """include/rt_api.h rt_upscale_params: the two frames' jitters (render pixels), max_history (1..1024), depth_tol."""
    _fields_ = [("jitter_cur", ctypes.c_float * 2), ("jitter_prev", ctypes.c_float * 2),
                ("max_history", ctypes.c_uint32), ("depth_tol", ctypes.c_float)]


class rt_tile_plan_args(ctypes.Structure):
    """include/rt_api.h rt_tile_plan_args: the plan kernel's knobs for rt_tile_plan_probe."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("ntiles", "extra_cap", "slots", "kmax_code", "force", "split", "front",
                                               "prio", "min_gain", "waves_per_frame", "grid_x", "wx", "wy", "wl")]


class rt_manipulator(ctypes.Structure):
    """include/rt_api.h rt_manipulator: nv_helpers_dx12::Manipulator state (manipulator.h:124-144)."""
    _fields_ = [("pos", ctypes.c_float * 3), ("interest", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
                ("roll", ctypes.c_float), ("matrix", ctypes.c_float * 16), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("speed", ctypes.c_float), ("mouse", ctypes.c_float * 2),
                ("tbsize", ctypes.c_float), ("mode", ctypes.c_int32)]


_P = ctypes.c_void_p
_U32 = ctypes.c_uint32
_I = ctypes.c_int
_FP = ctypes.POINTER(ctypes.c_float)
_UP = ctypes.POINTER(ctypes.c_uint32)

# (name, restype, argtypes) — every function declared in include/rt_api.h
SIGNATURES = [
    ("rt_api_version", _I, []),
    ("rt_status_string", ctypes.c_char_p, [_I]),
    ("rt_last_error", ctypes.c_char_p, [_P]),
    ("rt_create", _I, [_I, ctypes.POINTER(_P)]),
    ("rt_destroy", _I, [_P]),
    ("rt_blas_build", _I, [_P, _P, _U32, _U32, _P, _U32, _UP]),
    ("rt_blas_rebuild", _I, [_P, _U32, _P, _U32, _U32, _P, _U32]),
    ("rt_blas_refit", _I, [_P, _U32, _P, _U32, _U32]),
    ("rt_blas_refit_device", _I, [_P, _U32, _P, _U32, _U32, _P]),
    ("rt_blas_info", _I, [_P, _U32, ctypes.POINTER(rt_bvh_info)]),
    ("rt_blas_export", _I, [_P, _U32, _P, ctypes.c_size_t, _P, ctypes.c_size_t]),
    ("rt_tlas_build", _I, [_P, ctypes.POINTER(rt_instance), _U32, _I]),
    ("rt_tlas_info", _I, [_P, ctypes.POINTER(rt_bvh_info)]),
    ("rt_tlas_build_wall_ms", ctypes.c_double, [_P]),
    ("rt_tlas_export", _I, [_P, _P, ctypes.c_size_t]),
    ("rt_set_camera", _I, [_P, _FP]),
    ("rt_set_shading", _I, [_P, ctypes.POINTER(rt_light), _U32, ctypes.POINTER(rt_material), _I, _I]),
    ("rt_set_schedule", _I, [_P, _I]),
    ("rt_set_tile_rows", _I, [_P, _I]),
    ("rt_set_tile_balance", _I, [_P, _I]),
    ("rt_tile_balance_info", _I, [_P, _UP]),
    ("rt_tile_balance_info_n", _I, [_P, _UP, _U32]),
    ("rt_ctx_counters", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("rt_ctx_counters_n", _I, [_P, ctypes.POINTER(ctypes.c_uint64), _U32]),
    ("rt_tile_plan_probe", _I, [_P, ctypes.POINTER(rt_tile_plan_args), _UP, _UP, _U32, _UP, _U32, _UP]),
    ("rt_set_triangle_test", _I, [_P, _I]),
    ("rt_set_stats", _I, [_P, _I]),
    ("rt_dispatch_rays", _I, [_P, _U32, _U32, _P, _U32, _P, _P, _P]),
    ("rt_dispatch_frames", _I, [_P, _U32, _U32, _U32, _P, _P, ctypes.c_uint64, _P]),
    ("rt_dispatch_gbuffer", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_gbuffer), _P]),
    ("rt_set_motion_history", _I, [_P, _I]),
    ("rt_dispatch_gbuffer_motion", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_gbuffer_motion), _FP, _P]),
    ("rt_dispatch_rays_gbuffer", _I, [_P, _U32, _U32, _P, _U32, _P, _P, ctypes.POINTER(rt_gbuffer_motion), _FP, _P]),
    ("rt_dispatch_ao", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_ao_params), _P, _P]),
    ("rt_dispatch_shadow", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_shadow_params), _P, ctypes.c_uint64, _P]),
    ("rt_shade_resolve", _I, [_P, _U32, _U32, ctypes.POINTER(rt_resolve_inputs), _P, _P, _P]),
    ("rt_shade_resolve_pbr", _I, [_P, _U32, _U32, ctypes.POINTER(rt_resolve_pbr_inputs),
                                  ctypes.POINTER(rt_material_table), _P, _P, _P]),
    ("rt_dispatch_reflection", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_reflection_params),
                                    ctypes.POINTER(rt_reflection_planes), _P]),
    ("rt_dispatch_reflection_pbr", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_reflection_pbr_params),
                                        ctypes.POINTER(rt_material_table), ctypes.POINTER(rt_reflection_planes), _P]),
    ("rt_dispatch_reflection_chain", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_reflection_chain_params),
                                          ctypes.POINTER(rt_material_table), ctypes.POINTER(rt_reflection_planes),
                                          _P]),
    ("rt_dispatch_indirect", _I, [_P, _U32, _U32, _P, _U32, ctypes.POINTER(rt_indirect_params),
                                  ctypes.POINTER(rt_material_table), ctypes.POINTER(rt_reflection_planes), _P]),
    ("rt_shade_resolve_gi", _I, [_P, _U32, _U32, ctypes.POINTER(rt_resolve_gi_inputs),
                                 ctypes.POINTER(rt_material_table), _P, _P, _P]),
    ("rt_reflection_composite", _I, [_P, _U32, _U32, ctypes.POINTER(rt_reflection_composite_params), _P, _P, _P, _P,
                                     _P, _P, _P]),
    ("rt_denoise_guide", _I, [_P, _U32, _P, _P, _U32, _P, _P]),
    ("rt_ao_accumulate", _I, [_P, _U32, _U32, ctypes.POINTER(rt_ao_temporal_params), _P, _P, _P, _P, _P, _P, _P, _P,
                              _P]),
    ("rt_ao_atrous", _I, [_P, _U32, _U32, ctypes.POINTER(rt_ao_atrous_params), _P, _P, _P, _P, _P]),
    ("rt_ao_accumulate_planes", _I, [_P, _U32, _U32, ctypes.POINTER(rt_ao_temporal_params), _U32, _P, _P, _P, _P, _P,
                                     _P, _P, _P, _P]),
    ("rt_ao_atrous_planes", _I, [_P, _U32, _U32, ctypes.POINTER(rt_ao_atrous_params), _U32, _P, _P, _P, _P, _P]),
    ("rt_radiance_accumulate", _I, [_P, _U32, _U32, ctypes.POINTER(rt_radiance_temporal_params), _P, _P, _P, _P, _P,
                                    _P, _P, _P, _P]),
    ("rt_radiance_atrous", _I, [_P, _U32, _U32, ctypes.POINTER(rt_radiance_atrous_params), _P, _P, _P, _P, _P, _P, _P,
                                _P]),
    ("rt_reflection_motion", _I, [_P, _U32, _U32, ctypes.POINTER(rt_reflection_motion_params), _P, _P, _P, _P, _U32,
                                  _P, _P, _P, _P, _P, _P]),
    ("rt_radiance_accumulate_reflection", _I, [_P, _U32, _U32, ctypes.POINTER(rt_radiance_temporal_params),
                                               ctypes.POINTER(rt_reflection_motion_params), _P, _P, _P, _P, _P, _P, _P,
                                               _P, _P, _P, _P, _P]),
    ("rt_upscale", _I, [_P, _U32, _U32, _U32, _U32, ctypes.POINTER(rt_upscale_params), _P, _P, _P, _P, _P, _P, _P, _P,
                        _P]),
    ("rt_trace_rays", _I, [_P, _P, _U32, _U32, _P, _P, _P]),
    ("rt_raster_draw", _I, [_P, _UP, _U32, _FP, _U32, _U32, _P, _P, _P]),
    ("rt_assemble_strips", _I, [_P, _U32, _U32, _U32, _U32, _P, _P, _P]),
    ("rt_strip_rows", _U32, [_U32, _U32, _U32, _U32, _P, _U32]),
    ("rt_forget_stream", _I, [_P, _P]),
    ("rt_event_create", _I, [ctypes.POINTER(_P)]),
    ("rt_event_destroy", _I, [_P]),
    ("rt_event_record", _I, [_P, _P]),
    ("rt_stream_wait_event", _I, [_P, _P]),
    ("rt_comm_available", _I, []),
    ("rt_comm_get_unique_id", _I, [_P]),
    ("rt_comm_init", _I, [_P, _U32, _U32, _P, ctypes.POINTER(_P)]),
    ("rt_comm_init_loopback", _I, [_P, _U32, ctypes.POINTER(_P)]),
    ("rt_comm_destroy", _I, [_P]),
    ("rt_comm_abort", _I, [_P]),
    ("rt_comm_loopback_render_ranks", _I, [_P, _U32, _U32]),
    ("rt_comm_set_phase_timing", _I, [_P, ctypes.c_int]),
    ("rt_comm_phase_stats", _I, [_P, ctypes.POINTER(ctypes.c_double), _U32]),
    ("rt_comm_last_error", ctypes.c_char_p, [_P]),
    ("rt_comm_stream", _P, [_P]),
    ("rt_comm_synchronize", _I, [_P]),
    ("rt_render_strips", _I, [_P, _U32, _U32, _U32, _P, _P]),
    ("rt_render_strips_frames", _I, [_P, _U32, _U32, _U32, _U32, _FP, ctypes.POINTER(_P), _P]),
    ("rt_comm_pipeline_depth", _U32, [_P]),
    ("rt_comm_set_batch", _I, [_P, _U32]),
    ("rt_comm_batch", _U32, [_P]),
    ("rt_stats", _I, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    ("rt_stats_reset", _I, [_P]),
    ("rt_mesh_load_obj", _I, [ctypes.c_char_p, ctypes.POINTER(_P)]),
    ("rt_mesh_parse_obj", _I, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_P)]),
    ("rt_mesh_free", None, [_P]),
    ("rt_mesh_vertex_count", _U32, [_P]),
    ("rt_mesh_index_count", _U32, [_P]),
    ("rt_mesh_vertices", _FP, [_P]),
    ("rt_mesh_indices", _UP, [_P]),
    ("rt_mesh_compute_vertex_normals", _I, [_P]),
    ("rt_plane_vertices", None, [_FP]),
    ("rt_camera_lookat", None, [_FP, _FP, _FP, _FP]),
    ("rt_camera_buffer", None, [_FP, _U32, _U32, ctypes.c_float, ctypes.c_float, ctypes.c_float, _FP]),
    ("rt_host_trace_triangles", _I, [_P, _U32, _U32, _P, _U32, _P, _P, _U32, _U32, _I, _P, _P]),
    ("rt_host_shading_normals", _I, [_P, _U32, _U32, _P, _U32, _P, _U32, _P, _P, _U32, _P]),
    ("rt_host_motion_project", _I, [_P, _P, _U32, _P, _P, _U32, _U32, _P]),
    ("rt_host_motion_vectors", _I, [_P, _P, _U32, _U32, _P, _U32, _P, _P, _P, _P, _U32, _U32, _P, _P, _U32, _P]),
    ("rt_host_ao_rays", _I, [_P, _P, _P, _P, _P, _U32, ctypes.POINTER(rt_ao_params), _P, _P]),
    ("rt_host_shadow_rays", _I, [_P, _P, _P, _P, _P, _P, _U32, ctypes.POINTER(rt_light), _U32,
                                 ctypes.POINTER(rt_shadow_params), _P, _P]),
    ("rt_host_shade_resolve", _I, [_U32, _U32, _FP, ctypes.POINTER(rt_light), _U32, ctypes.POINTER(rt_resolve_inputs),
                                   _P, _P]),
    ("rt_host_shade_resolve_pbr", _I, [_U32, _U32, _FP, ctypes.POINTER(rt_light), _U32,
                                       ctypes.POINTER(rt_resolve_pbr_inputs), ctypes.POINTER(rt_material_table), _P,
                                       _P]),
    ("rt_host_reflection_rays", _I, [_P, _P, _P, _P, _P, _U32, ctypes.POINTER(rt_reflection_params), _P, _P]),
    ("rt_host_reflection_radiance", _I, [_P, _P, _P, _P, _P, _P, _P, _U32, _U32, ctypes.POINTER(rt_light), _U32,
                                         ctypes.POINTER(rt_reflection_params), _P, _P]),
    ("rt_host_reflection_rays_flags", _I, [_P, _P, _P, _P, _P, _U32, ctypes.POINTER(rt_reflection_pbr_params), _P,
                                           _P]),
    ("rt_host_reflection_radiance_pbr", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _U32, _U32, ctypes.POINTER(rt_light), _U32,
                                             ctypes.POINTER(rt_reflection_pbr_params),
                                             ctypes.POINTER(rt_material_table), _P, _P]),
    ("rt_host_reflection_chain_rays", _I, [_P, _P, _P, _P, _P, _U32, ctypes.c_float,
                                           ctypes.POINTER(rt_material_table), _P, _P]),
    ("rt_host_reflection_chain_radiance", _I, [_U32, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _U32,
                                               ctypes.POINTER(rt_light), _U32,
                                               ctypes.POINTER(rt_reflection_chain_params),
                                               ctypes.POINTER(rt_material_table), _P, _P, _P]),
    ("rt_host_last_error", ctypes.c_char_p, []),
    ("rt_host_reflection_composite", _I, [_U32, _U32, _FP, ctypes.POINTER(rt_reflection_composite_params), _P, _P, _P,
                                          _P, _P, _P]),
    ("rt_host_indirect_rays", _I, [_P, _P, _P, _P, _P, _U32, ctypes.POINTER(rt_indirect_params), _P, _P]),
    ("rt_host_shade_resolve_gi", _I, [_U32, _U32, _FP, ctypes.POINTER(rt_light), _U32,
                                      ctypes.POINTER(rt_resolve_gi_inputs), ctypes.POINTER(rt_material_table), _P,
                                      _P]),
    ("rt_host_denoise_guide", _I, [_U32, _P, _P, _U32, _P]),
    ("rt_host_ao_accumulate", _I, [_U32, _U32, ctypes.POINTER(rt_ao_temporal_params), _P, _P, _P, _P, _P, _P, _P, _P]),
    ("rt_host_ao_atrous", _I, [_U32, _U32, ctypes.POINTER(rt_ao_atrous_params), _P, _P, _P, _P]),
    ("rt_host_ao_accumulate_planes", _I, [_U32, _U32, ctypes.POINTER(rt_ao_temporal_params), _U32, _P, _P, _P, _P, _P,
                                          _P, _P, _P]),
    ("rt_host_ao_atrous_planes", _I, [_U32, _U32, ctypes.POINTER(rt_ao_atrous_params), _U32, _P, _P, _P, _P]),
    ("rt_host_radiance_accumulate", _I, [_U32, _U32, ctypes.POINTER(rt_radiance_temporal_params), _P, _P, _P, _P, _P,
                                         _P, _P, _P]),
    ("rt_host_radiance_atrous", _I, [_U32, _U32, ctypes.POINTER(rt_radiance_atrous_params), _P, _P, _P, _P, _P, _P,
                                     _P]),
    ("rt_host_reflection_motion", _I, [_U32, _U32, ctypes.POINTER(rt_reflection_motion_params), _P, _P, _P, _P, _U32,
                                       _P, _P, _P, _P, _P]),
    ("rt_host_upscale", _I, [_U32, _U32, _U32, _U32, ctypes.POINTER(rt_upscale_params), _P, _P, _P, _P, _P, _P, _P,
                             _P]),
    ("rt_camera_jitter", _I, [_FP, _U32, _U32, ctypes.c_float, ctypes.c_float, _FP]),
    ("rt_jitter_halton", _I, [_U32, _FP]),
    ("rt_manip_init", None, [ctypes.POINTER(rt_manipulator)]),
    ("rt_manip_update", None, [ctypes.POINTER(rt_manipulator)]),
    ("rt_manip_set_lookat", None, [ctypes.POINTER(rt_manipulator), _FP, _FP, _FP]),
    ("rt_manip_set_roll", None, [ctypes.POINTER(rt_manipulator), ctypes.c_float]),
    ("rt_manip_set_window_size", None, [ctypes.POINTER(rt_manipulator), ctypes.c_int32, ctypes.c_int32]),
    ("rt_manip_set_mouse_position", None, [ctypes.POINTER(rt_manipulator), ctypes.c_int32, ctypes.c_int32]),
    ("rt_manip_motion", None, [ctypes.POINTER(rt_manipulator), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    ("rt_manip_mouse_move", ctypes.c_int32, [ctypes.POINTER(rt_manipulator), ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_uint32]),
    ("rt_manip_wheel", None, [ctypes.POINTER(rt_manipulator), ctypes.c_int32]),
]


def _load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Loads the C-ABI library (a variant build may be given for A/B timing in one process)."""
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()' or `make`). There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def _status_name(st: int) -> str:
    return lib.rt_status_string(st).decode()


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(_FP)


def _f32(x, n=None) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} floats, got {a.size}")
    return a


# ---------------------------------------------------------------------------------------------
# host services (no GPU)
# ---------------------------------------------------------------------------------------------

class Mesh:
    """OBJFileManager::LoadObjFile result (OBJ_FileManager.cpp:10-71) held by the C library."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load_obj(cls, path: str) -> "Mesh":
        h = _P()
        st = lib.rt_mesh_load_obj(path.encode(), ctypes.byref(h))
        if st != RT_OK:
            raise RtError(st, f"cannot load {path}")
        return cls(h)

    @classmethod
    def parse_obj(cls, text: bytes) -> "Mesh":
        h = _P()
        st = lib.rt_mesh_parse_obj(text, len(text), ctypes.byref(h))
        if st != RT_OK:
            raise RtError(st, "parse failed")
        return cls(h)

    @classmethod
    def asset(cls, name: str) -> "Mesh":
        """A model shipped with the package (teapot, rabbit), stored gzip-compressed."""
        with gzip.open(os.path.join(ASSETS, f"{name}.obj.gz"), "rb") as f:
            return cls.parse_obj(f.read())

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.rt_mesh_free(self._h)
            self._h = None

    @property
    def vertex_count(self) -> int:
        return lib.rt_mesh_vertex_count(self._h)

    @property
    def index_count(self) -> int:
        return lib.rt_mesh_index_count(self._h)

    @property
    def vertices(self) -> np.ndarray:
        n = self.vertex_count
        if n == 0:
            return np.zeros((0, 6), np.float32)
        return np.ctypeslib.as_array(lib.rt_mesh_vertices(self._h), shape=(n * 6,)).reshape(n, 6).copy()

    @property
    def indices(self) -> np.ndarray:
        n = self.index_count
        if n == 0:
            return np.zeros((0,), np.uint32)
        return np.ctypeslib.as_array(lib.rt_mesh_indices(self._h), shape=(n,)).copy()

    def compute_vertex_normals(self) -> "Mesh":
        st = lib.rt_mesh_compute_vertex_normals(self._h)
        if st != RT_OK:
            raise RtError(st, "ComputeVertexNormals")
        return self


def plane_vertices() -> np.ndarray:
    out = np.zeros(36, np.float32)
    lib.rt_plane_vertices(_fptr(out))
    return out.reshape(6, 6)


def camera_lookat(eye, center, up) -> np.ndarray:
    e, c, u = _f32(eye, 3), _f32(center, 3), _f32(up, 3)
    out = np.zeros(16, np.float32)
    lib.rt_camera_lookat(_fptr(e), _fptr(c), _fptr(u), _fptr(out))
    return out


def camera_buffer(view, width: int, height: int, fov_deg: float = 45.0, znear: float = 0.1,
                  zfar: float = 1000.0) -> np.ndarray:
    v = _f32(view, 16)
    out = np.zeros(64, np.float32)
    lib.rt_camera_buffer(_fptr(v), width, height, fov_deg, znear, zfar, _fptr(out))
    return out


def host_trace_triangles(vertices, indices, rays, triangle_test: int = RT_TRIANGLE_TEST_MOLLER_TRUMBORE,
                         object_to_world=None, any_hit: bool = False, cull_back: bool = False,
                         cull_front: bool = False):
    """rt_host_trace_triangles: rt_trace_rays on the host, brute force over one mesh under one instance transform
    (no GPU). vertices: (nv, k >= 3) floats, position first; indices: uint32 triangle list or None; rays: (n, 8)
    floats (o, tmin, d, tmax); object_to_world: 12 floats (3x4 row-major) or None. Returns (hits (n, 4) uint32:
    t bits, instance 0, primitive, flag; uv (n, 2) float32)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    if v.ndim != 2:
        v = v.reshape(-1, 6)
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    n = r.shape[0]
    i = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).ravel()
    x = None if object_to_world is None else _f32(object_to_world, 12)
    flags = (RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH if any_hit else 0) | \
        (RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES if cull_back else 0) | \
        (RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES if cull_front else 0)
    hits = np.zeros((n, 4), np.uint32)
    uv = np.zeros((n, 2), np.float32)
    st = lib.rt_host_trace_triangles(v.ctypes.data_as(_P), v.shape[0], v.shape[1] * 4,
                                     None if i is None else i.ctypes.data_as(_P), 0 if i is None else i.size,
                                     None if x is None else x.ctypes.data_as(_P), r.ctypes.data_as(_P), n, flags,
                                     triangle_test, hits.ctypes.data_as(_P), uv.ctypes.data_as(_P))
    if st != RT_OK:
        raise RtError(st, "rt_host_trace_triangles")
    return hits, uv


def host_shading_normals(vertices, indices, prims, uv, hit_group: int = RT_HITGROUP_MODEL, object_to_world=None):
    """rt_host_shading_normals: the G-buffer's normal plane on the host (no GPU), for hits on one mesh under one
    instance transform. vertices: (nv, k >= 6) floats {pos, normal, ..}; indices: uint32 triangle list or None; prims:
    n primitive indices; uv: (n, 2) barycentrics; hit_group: RT_HITGROUP_MODEL or RT_HITGROUP_PLANE; object_to_world:
    12 floats (3x4 row-major) or None. Returns (n, 4) float32 (w = 0)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    if v.ndim != 2:
        v = v.reshape(-1, 6)
    i = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).ravel()
    x = None if object_to_world is None else _f32(object_to_world, 12)
    p = np.ascontiguousarray(prims, dtype=np.uint32).ravel()
    b = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    if b.shape[0] != p.size:
        raise ValueError(f"expected {p.size} (u, v) pairs, got {b.shape[0]}")
    out = np.zeros((p.size, 4), np.float32)
    st = lib.rt_host_shading_normals(v.ctypes.data_as(_P), v.shape[0], v.shape[1] * 4,
                                     None if i is None else i.ctypes.data_as(_P), 0 if i is None else i.size,
                                     None if x is None else x.ctypes.data_as(_P), hit_group, p.ctypes.data_as(_P),
                                     b.ctypes.data_as(_P), p.size, out.ctypes.data_as(_P))
    if st != RT_OK:
        raise RtError(st, "rt_host_shading_normals")
    return out


def _vp(a):
    return None if a is None else a.ctypes.data_as(_P)


def host_motion_project(points, prev_points, camera, prev_camera, width: int, height: int):
    """rt_host_motion_project: the motion plane's projection stage on the host (no GPU). points / prev_points: (n, 3)
    world points now and in the previous frame; camera / prev_camera: 64-float camera buffers (prev_camera None: the
    same camera). Returns (n, 4) float32: mx, my, w_prev, w_cur (rt_dispatch_gbuffer_motion)."""
    a = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(prev_points, dtype=np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"expected {a.shape[0]} previous points, got {b.shape[0]}")
    cb = _f32(camera, 64)
    pcb = None if prev_camera is None else _f32(prev_camera, 64)
    out = np.zeros((a.shape[0], 4), np.float32)
    st = lib.rt_host_motion_project(_vp(a), _vp(b), a.shape[0], _vp(cb), _vp(pcb), width, height, _vp(out))
    if st != RT_OK:
        raise RtError(st, "rt_host_motion_project")
    return out


def host_motion_vectors(vertices, indices, prims, uv, camera, width: int, height: int, prev_vertices=None,
                        object_to_world=None, prev_object_to_world=None, prev_camera=None):
    """rt_host_motion_vectors: the motion plane on the host (no GPU) for hits on one mesh under one instance.
    vertices: (nv, k >= 3) floats; prev_vertices: the same layout or None (= vertices); indices: uint32 triangle list
    or None; prims: n primitive indices; uv: (n, 2) barycentrics; object_to_world / prev_object_to_world: 12 floats
    or None (identity / the current one); camera / prev_camera: 64-float camera buffers (prev_camera None: the same).
    Returns (n, 4) float32: mx, my, w_prev, w_cur."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    if v.ndim != 2:
        v = v.reshape(-1, 6)
    pv = None
    if prev_vertices is not None:
        pv = np.ascontiguousarray(prev_vertices, dtype=np.float32).reshape(-1, v.shape[1])
        if pv.shape != v.shape:
            raise ValueError(f"previous vertices: expected shape {v.shape}, got {pv.shape}")
    i = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).ravel()
    x = None if object_to_world is None else _f32(object_to_world, 12)
    px = None if prev_object_to_world is None else _f32(prev_object_to_world, 12)
    cb = _f32(camera, 64)
    pcb = None if prev_camera is None else _f32(prev_camera, 64)
    p = np.ascontiguousarray(prims, dtype=np.uint32).ravel()
    b = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    if b.shape[0] != p.size:
        raise ValueError(f"expected {p.size} (u, v) pairs, got {b.shape[0]}")
    out = np.zeros((p.size, 4), np.float32)
    st = lib.rt_host_motion_vectors(_vp(v), _vp(pv), v.shape[0], v.shape[1] * 4, _vp(i), 0 if i is None else i.size,
                                    _vp(x), _vp(px), _vp(cb), _vp(pcb), width, height, _vp(p), _vp(b), p.size, _vp(out))
    if st != RT_OK:
        raise RtError(st, "rt_host_motion_vectors")
    return out


def host_ao_rays(cam_rays, t, normal, px, py, samples: int, radius: float, tmin: float = 0.01, seed: int = 0):
    """rt_host_ao_rays: the rays rt_dispatch_ao traces, on the host (no GPU). cam_rays: (n, 8) camera rays in
    trace_rays' layout; t: n hit distances; normal: (n, 4) G-buffer normals; px, py: the pixels' global coordinates.
    Returns (rays, valid): (n, samples, 8) float32 (P, tmin, d, radius) and (n,) uint8; a pixel whose normal is not
    valid has zero rays and valid 0."""
    cr = np.ascontiguousarray(cam_rays, dtype=np.float32).reshape(-1, 8)
    n = cr.shape[0]
    tt = _f32(t, n)
    nr = _f32(normal, 4 * n)
    x = np.ascontiguousarray(px, dtype=np.uint32).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if x.size != n or y.size != n:
        raise ValueError(f"expected {n} pixel coordinates, got {x.size} and {y.size}")
    if not 1 <= int(samples) <= 64:  # rt_host_ao_rays' own limit, checked before the output is sized by it
        raise RtError(RT_E_INVALID, f"rt_host_ao_rays: samples {samples} outside 1..64")
    p = rt_ao_params(samples, seed, radius, tmin)
    rays = np.zeros((n, int(samples), 8), np.float32)
    valid = np.zeros(n, np.uint8)
    st = lib.rt_host_ao_rays(_vp(cr), _vp(tt), _vp(nr), _vp(x), _vp(y), n, ctypes.byref(p), _vp(rays), _vp(valid))
    if st != RT_OK:
        raise RtError(st, "rt_host_ao_rays")
    return rays, valid


def _lights_array(lights):
    """An rt_light array from (colour, position, intensity) triples, Context.set_shading's form."""
    lights = list(lights)
    arr = (rt_light * len(lights))()
    for k, (col, pos, inten) in enumerate(lights):
        arr[k].color[:] = [float(v) for v in col]
        arr[k].position[:] = [float(v) for v in pos]
        arr[k].intensity = float(inten)
    return arr


def host_shadow_rays(cam_rays, t, normal, hit_group, px, py, lights, samples: int = 1, light_radius: float = 0.0,
                     tmin: float = 0.01, seed: int = 0):
    """rt_host_shadow_rays: the rays rt_dispatch_shadow traces, on the host (no GPU). cam_rays: (n, 8) camera rays in
    trace_rays' layout; t: n hit distances; normal: (n, 4) G-buffer normals; hit_group: n hit groups (the object
    plane's second word); px, py: the pixels' global coordinates; lights: set_shading's (colour, position, intensity)
    triples. Returns (rays, lit): (n, nlights, samples, 8) float32 (P, tmin, d, 100000) and (n, nlights) uint8; a pair
    that is not lit has zero rays and lit 0. Primary misses are the caller's to leave out."""
    cr = np.ascontiguousarray(cam_rays, dtype=np.float32).reshape(-1, 8)
    n = cr.shape[0]
    tt = _f32(t, n)
    nr = _f32(normal, 4 * n)
    g = np.ascontiguousarray(hit_group, dtype=np.uint32).ravel()
    x = np.ascontiguousarray(px, dtype=np.uint32).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if x.size != n or y.size != n or g.size != n:
        raise ValueError(f"expected {n} pixel coordinates and hit groups, got {x.size}, {y.size} and {g.size}")
    arr = _lights_array(lights)
    nl = len(arr)
    if not 1 <= int(samples) <= 64:  # rt_host_shadow_rays' own limits, checked before the output is sized by them
        raise RtError(RT_E_INVALID, f"rt_host_shadow_rays: samples {samples} outside 1..64")
    if not 1 <= nl <= 16:
        raise RtError(RT_E_INVALID, f"rt_host_shadow_rays: {nl} lights, outside 1..16")
    p = rt_shadow_params(samples, seed, light_radius, tmin)
    rays = np.zeros((n, nl, int(samples), 8), np.float32)
    lit = np.zeros((n, nl), np.uint8)
    st = lib.rt_host_shadow_rays(_vp(cr), _vp(tt), _vp(nr), _vp(g), _vp(x), _vp(y), n, arr, nl, ctypes.byref(p),
                                 _vp(rays), _vp(lit))
    if st != RT_OK:
        raise RtError(st, "rt_host_shadow_rays")
    return rays, lit


def host_shade_resolve(width: int, height: int, camera, lights, hits, normal, object, vis=None, ao=None,  # noqa: A002
                       want_rgba8: bool = False):
    """rt_host_shade_resolve: the deferred resolve on the host (no GPU). camera: the 64-float camera buffer; lights:
    set_shading's triples; hits (n, 4) uint32, normal (n, 4) float32, object (n, 2) uint32 with n = width * height;
    vis: (nlights, n) float32 or None (every light fully visible); ao: n float32 or None (1). Returns color (n, 4)
    float32 and, with want_rgba8, the (n, 4) uint8 frame as a second."""
    n = width * height
    cb = _f32(camera, 64)
    arr = _lights_array(lights)
    nl = len(arr)
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    oo = np.ascontiguousarray(object).view(np.uint32).reshape(-1)
    if hh.size != 4 * n or oo.size != 2 * n:
        raise ValueError(f"expected {4 * n} hit words and {2 * n} object words, got {hh.size} and {oo.size}")
    nn = _f32(normal, 4 * n)
    vv = None if vis is None else _f32(vis, nl * n)
    aa = None if ao is None else _f32(ao, n)
    inp = rt_resolve_inputs(_vp(hh), _vp(nn), _vp(oo), _vp(vv), 0, _vp(aa))
    out = np.zeros((n, 4), np.float32)
    out8 = np.zeros((n, 4), np.uint8) if want_rgba8 else None
    st = lib.rt_host_shade_resolve(width, height, _fptr(cb), arr, nl, ctypes.byref(inp), _vp(out), _vp(out8))
    if st != RT_OK:
        raise RtError(st, "rt_host_shade_resolve")
    return (out, out8) if want_rgba8 else out


def _materials_array(materials):
    """An rt_material array from 6-tuples (albedo rgb, roughness, metallic, reflectivity), set_shading's material
    format. The count is left to the library to refuse."""
    materials = [tuple(float(v) for v in m) for m in materials]
    arr = (rt_material * max(len(materials), 1))()
    for k, m in enumerate(materials):
        if len(m) != 6:
            raise ValueError(f"material {k}: expected 6 values (albedo rgb, roughness, metallic, reflectivity), got "
                             f"{len(m)}")
        arr[k].albedo[:] = m[0:3]
        arr[k].roughness, arr[k].metallic, arr[k].reflectivity = m[3:6]
    return arr, len(materials)


def host_shade_resolve_pbr(width: int, height: int, camera, lights, hits, normal, object, materials,  # noqa: A002
                           instance_material=None, vis=None, ao=None, refl=None, want_rgba8: bool = False):
    """rt_host_shade_resolve_pbr: the PBR resolve on the host (no GPU). camera, lights, hits, normal, object, vis, ao as
    host_shade_resolve; materials: a sequence of 6-tuples, set_shading's material format (1..32 of them);
    instance_material: uint32 material indices by instance index (object's first word), or None (material 0
    everywhere); refl: (n, 4) float32, the reflection pass's radiance plane, or None. Returns color (n, 4) float32 and,
    with want_rgba8, the (n, 4) uint8 frame as a second."""
    n = width * height
    cb = _f32(camera, 64)
    arr = _lights_array(lights)
    nl = len(arr)
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    oo = np.ascontiguousarray(object).view(np.uint32).reshape(-1)
    if hh.size != 4 * n or oo.size != 2 * n:
        raise ValueError(f"expected {4 * n} hit words and {2 * n} object words, got {hh.size} and {oo.size}")
    nn = _f32(normal, 4 * n)
    vv = None if vis is None else _f32(vis, nl * n)
    aa = None if ao is None else _f32(ao, n)
    rr = None if refl is None else _f32(refl, 4 * n)
    mats, nm = _materials_array(materials)
    im = None if instance_material is None else np.ascontiguousarray(instance_material, dtype=np.uint32).ravel()
    inp = rt_resolve_pbr_inputs(_vp(hh), _vp(nn), _vp(oo), _vp(vv), 0, _vp(aa), _vp(rr))
    table = rt_material_table(mats, nm, _vp(im), 0 if im is None else im.size)
    out = np.zeros((n, 4), np.float32)
    out8 = np.zeros((n, 4), np.uint8) if want_rgba8 else None
    st = lib.rt_host_shade_resolve_pbr(width, height, _fptr(cb), arr, nl, ctypes.byref(inp), ctypes.byref(table),
                                       _vp(out), _vp(out8))
    if st != RT_OK:
        raise RtError(st, "rt_host_shade_resolve_pbr")
    return (out, out8) if want_rgba8 else out


def host_reflection_rays(cam_rays, t, normal, px, py, samples: int = 1, roughness: float = 0.0, tmax: float = 1000.0,
                         shadow_tmin: float = 0.01, seed: int = 0):
    """rt_host_reflection_rays: the rays rt_dispatch_reflection traces, on the host (no GPU). cam_rays: (n, 8) camera
    rays in trace_rays' layout; t: n hit distances; normal: (n, 4) G-buffer normals; px, py: the pixels' global
    coordinates. Returns (rays, valid): (n, samples, 8) float32 (P + 0.001 d, 0.001, d, tmax), to be traced closest-hit
    with cull_back, and n uint8; an invalid normal has zero rays and valid 0. Primary misses are the caller's to leave
    out."""
    cr = np.ascontiguousarray(cam_rays, dtype=np.float32).reshape(-1, 8)
    n = cr.shape[0]
    tt = _f32(t, n)
    nr = _f32(normal, 4 * n)
    x = np.ascontiguousarray(px, dtype=np.uint32).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if x.size != n or y.size != n:
        raise ValueError(f"expected {n} pixel coordinates, got {x.size} and {y.size}")
    if not 1 <= int(samples) <= 64:  # rt_host_reflection_rays' own limit, checked before the output is sized by it
        raise RtError(RT_E_INVALID, f"rt_host_reflection_rays: samples {samples} outside 1..64")
    p = rt_reflection_params(samples, seed, roughness, tmax, shadow_tmin)
    rays = np.zeros((n, int(samples), 8), np.float32)
    valid = np.zeros(n, np.uint8)
    st = lib.rt_host_reflection_rays(_vp(cr), _vp(tt), _vp(nr), _vp(x), _vp(y), n, ctypes.byref(p), _vp(rays),
                                     _vp(valid))
    if st != RT_OK:
        raise RtError(st, "rt_host_reflection_rays")
    return rays, valid


def host_reflection_radiance(rays, hits, hit_normal, hit_group, occluded, valid, py, height: int, lights,
                             roughness: float = 0.0, tmax: float = 1000.0, shadow_tmin: float = 0.01, seed: int = 0,
                             want_lit: bool = False):
    """rt_host_reflection_radiance: rt_dispatch_reflection's radiance plane from what its rays found, on the host (no
    GPU). rays: (n, S, 8) from host_reflection_rays; hits: (n, S, 4) uint32 records of their closest-hit trace;
    hit_normal: (n, S, 4) G-buffer-form normals of those hits; hit_group: (n, S) hit groups; occluded: (n, S, nlights)
    bytes, non-zero where the shadow ray of (hit, light) is occluded (read only where the hit faces the light); valid: n
    bytes; py: n global rows; height: the frame's; lights: set_shading's triples. Returns (n, 4) float32 (mean colour,
    mean distance) and, with want_lit, the (n, S, nlights) uint8 mask of the shadow rays traced."""
    ry = np.ascontiguousarray(rays, dtype=np.float32)
    if ry.ndim != 3 or ry.shape[2] != 8:
        raise ValueError(f"rays must be (n, samples, 8), got {ry.shape}")
    n, S = ry.shape[0], ry.shape[1]
    arr = _lights_array(lights)
    nl = len(arr)
    if not 1 <= S <= 64:
        raise RtError(RT_E_INVALID, f"rt_host_reflection_radiance: samples {S} outside 1..64")
    if not 1 <= nl <= 16:
        raise RtError(RT_E_INVALID, f"rt_host_reflection_radiance: {nl} lights, outside 1..16")
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    hn = _f32(hit_normal, 4 * n * S)
    hg = np.ascontiguousarray(hit_group, dtype=np.uint32).ravel()
    oc = np.ascontiguousarray(occluded, dtype=np.uint8).ravel()
    va = np.ascontiguousarray(valid, dtype=np.uint8).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if hh.size != 4 * n * S or hg.size != n * S or oc.size != n * S * nl or va.size != n or y.size != n:
        raise ValueError(f"expected {n} x {S} records and hit groups, {n * S * nl} occlusion bytes and {n} valid bytes "
                         f"and rows, got {hh.size // 4}, {hg.size}, {oc.size}, {va.size} and {y.size}")
    p = rt_reflection_params(S, seed, roughness, tmax, shadow_tmin)
    out = np.zeros((n, 4), np.float32)
    lit = np.zeros((n, S, nl), np.uint8) if want_lit else None
    st = lib.rt_host_reflection_radiance(_vp(ry), _vp(hh), _vp(hn), _vp(hg), _vp(oc), _vp(va), _vp(y), n, height, arr,
                                         nl, ctypes.byref(p), _vp(out), _vp(lit))
    if st != RT_OK:
        raise RtError(st, "rt_host_reflection_radiance")
    return (out, lit) if want_lit else out


def host_reflection_rays_flags(cam_rays, t, normal, px, py, samples: int = 1, roughness: float = 0.0,
                               tmax: float = 1000.0, shadow_tmin: float = 0.01, seed: int = 0, flags: int = 0):
    """rt_host_reflection_rays_flags: the rays rt_dispatch_reflection_pbr traces, on the host (no GPU):
    host_reflection_rays' arguments and results, and the pass's flags (RT_REFLECT_FRAME_RAY: the frame kernels' mirror
    direction, about the normal as stored). With flags 0 the bytes are host_reflection_rays'."""
    cr = np.ascontiguousarray(cam_rays, dtype=np.float32).reshape(-1, 8)
    n = cr.shape[0]
    tt = _f32(t, n)
    nr = _f32(normal, 4 * n)
    x = np.ascontiguousarray(px, dtype=np.uint32).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if x.size != n or y.size != n:
        raise ValueError(f"expected {n} pixel coordinates, got {x.size} and {y.size}")
    if not 1 <= int(samples) <= 64:  # the function's own limit, checked before the output is sized by it
        raise RtError(RT_E_INVALID, f"rt_host_reflection_rays_flags: samples {samples} outside 1..64")
    p = rt_reflection_pbr_params(samples, seed, roughness, tmax, shadow_tmin, flags)
    rays = np.zeros((n, int(samples), 8), np.float32)
    valid = np.zeros(n, np.uint8)
    st = lib.rt_host_reflection_rays_flags(_vp(cr), _vp(tt), _vp(nr), _vp(x), _vp(y), n, ctypes.byref(p), _vp(rays),
                                           _vp(valid))
    if st != RT_OK:
        raise RtError(st, "rt_host_reflection_rays_flags")
    return rays, valid


def host_reflection_radiance_pbr(rays, hits, hit_normal, hit_group, hit_inst, occluded, valid, py, height: int, lights,
                                 materials, instance_material=None, roughness: float = 0.0, tmax: float = 1000.0,
                                 shadow_tmin: float = 0.01, seed: int = 0, flags: int = 0, want_lit: bool = False):
    """rt_host_reflection_radiance_pbr: rt_dispatch_reflection_pbr's radiance plane from what its rays found, on the
    host (no GPU). host_reflection_radiance's arguments, and hit_inst: (n, S) instance indices of the hits; materials:
    a sequence of 6-tuples (1..32); instance_material: uint32 material indices by instance index, or None. occluded is
    read at light 0 of every plane hit and, with RT_REFLECT_SHADOW_MODELS, where a model hit faces the light. Returns
    (n, 4) float32 and, with want_lit, the (n, S, nlights) uint8 mask of the shadow rays the pass traces."""
    ry = np.ascontiguousarray(rays, dtype=np.float32)
    if ry.ndim != 3 or ry.shape[2] != 8:
        raise ValueError(f"rays must be (n, samples, 8), got {ry.shape}")
    n, S = ry.shape[0], ry.shape[1]
    arr = _lights_array(lights)
    nl = len(arr)
    if not 1 <= S <= 64:
        raise RtError(RT_E_INVALID, f"rt_host_reflection_radiance_pbr: samples {S} outside 1..64")
    if not 1 <= nl <= 16:
        raise RtError(RT_E_INVALID, f"rt_host_reflection_radiance_pbr: {nl} lights, outside 1..16")
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    hn = _f32(hit_normal, 4 * n * S)
    hg = np.ascontiguousarray(hit_group, dtype=np.uint32).ravel()
    hi = np.ascontiguousarray(hit_inst, dtype=np.uint32).ravel()
    oc = np.ascontiguousarray(occluded, dtype=np.uint8).ravel()
    va = np.ascontiguousarray(valid, dtype=np.uint8).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if hh.size != 4 * n * S or hg.size != n * S or hi.size != n * S or oc.size != n * S * nl or va.size != n \
            or y.size != n:
        raise ValueError(f"expected {n} x {S} records, hit groups and instances, {n * S * nl} occlusion bytes and {n} "
                         f"valid bytes and rows, got {hh.size // 4}, {hg.size}, {hi.size}, {oc.size}, {va.size} and "
                         f"{y.size}")
    mats, nm = _materials_array(materials)
    im = None if instance_material is None else np.ascontiguousarray(instance_material, dtype=np.uint32).ravel()
    table = rt_material_table(mats, nm, _vp(im), 0 if im is None else im.size)
    p = rt_reflection_pbr_params(S, seed, roughness, tmax, shadow_tmin, flags)
    out = np.zeros((n, 4), np.float32)
    lit = np.zeros((n, S, nl), np.uint8) if want_lit else None
    st = lib.rt_host_reflection_radiance_pbr(_vp(ry), _vp(hh), _vp(hn), _vp(hg), _vp(hi), _vp(oc), _vp(va), _vp(y), n,
                                             height, arr, nl, ctypes.byref(p), ctypes.byref(table), _vp(out), _vp(lit))
    if st != RT_OK:
        raise RtError(st, "rt_host_reflection_radiance_pbr")
    return (out, lit) if want_lit else out


def _host_table(materials, instance_material):
    """The rt_material_table of a host twin from set_shading-format materials and a host map (or None); the returned
    arrays must outlive the call."""
    mats, nm = _materials_array(materials)
    im = None if instance_material is None else np.ascontiguousarray(instance_material, dtype=np.uint32).ravel()
    return rt_material_table(mats, nm, _vp(im), 0 if im is None else im.size), (mats, im)


def host_reflection_chain_rays(rays, hits, hit_normal, hit_group, hit_inst, materials, instance_material=None,
                               tmax: float = 1000.0):
    """rt_host_reflection_chain_rays: the continuation rays of rt_dispatch_reflection_chain, on the host (no GPU).
    rays: (..., 8) traced rays; hits: (..., 4) uint32 records of their closest-hit search; hit_normal: (..., 4)
    stored-form normals of those hits; hit_group, hit_inst: (...) hit groups and instance indices; materials,
    instance_material: as for host_reflection_radiance_pbr. Returns rays (same shape; the frame kernels' reflection
    ray where the hit is a model hit whose material reflects, zeros elsewhere) and the uint8 mask of those hits. The
    bounce cap is the caller's loop."""
    ry = np.ascontiguousarray(rays, dtype=np.float32)
    if ry.ndim < 1 or ry.shape[-1] != 8:
        raise ValueError(f"rays must be (..., 8), got {ry.shape}")
    m = ry.size // 8
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    hn = _f32(hit_normal, 4 * m)
    hg = np.ascontiguousarray(hit_group, dtype=np.uint32).ravel()
    hi = np.ascontiguousarray(hit_inst, dtype=np.uint32).ravel()
    if hh.size != 4 * m or hg.size != m or hi.size != m:
        raise ValueError(f"expected {m} records, hit groups and instances, got {hh.size // 4}, {hg.size} and {hi.size}")
    table, _keep = _host_table(materials, instance_material)
    out = np.zeros(ry.shape, np.float32)
    cont = np.zeros(ry.shape[:-1], np.uint8)
    st = lib.rt_host_reflection_chain_rays(_vp(ry), _vp(hh), _vp(hn), _vp(hg), _vp(hi), m, tmax, ctypes.byref(table),
                                           _vp(out), _vp(cont))
    if st != RT_OK:
        raise RtError(st, lib.rt_host_last_error().decode() or "rt_host_reflection_chain_rays")
    return out, cont


def host_reflection_chain_radiance(rays, hits, hit_normal, hit_group, hit_inst, occluded, valid, py, height: int,
                                   lights, materials, instance_material=None, max_bounces: int = 4,
                                   roughness: float = 0.0, tmax: float = 1000.0, shadow_tmin: float = 0.01,
                                   seed: int = 0, flags: int = 0, want_lit: bool = False, want_nrays: bool = False):
    """rt_host_reflection_chain_radiance: rt_dispatch_reflection_chain's radiance plane from what the rays of every
    level found, on the host (no GPU): host_reflection_radiance_pbr's arguments with a leading level axis. rays:
    (levels, n, S, 8), level 0 the pass's first rays, level b + 1 host_reflection_chain_rays' rays of level b; hits,
    hit_normal: (levels, n, S, 4); hit_group, hit_inst: (levels, n, S); occluded: (levels, n, S, nlights); valid, py:
    (n,). An entry of a level is read only where its chain reaches that level. Returns (n, 4) float32 and, as asked,
    the (levels, n, S, nlights) uint8 mask of the shadow rays traced and the (n, S) uint8 rays of each chain. A chain
    that wants to go on past the supplied levels while below max_bounces raises RtError naming the pixel."""
    ry = np.ascontiguousarray(rays, dtype=np.float32)
    if ry.ndim != 4 or ry.shape[3] != 8:
        raise ValueError(f"rays must be (levels, n, samples, 8), got {ry.shape}")
    lv, n, S = ry.shape[0], ry.shape[1], ry.shape[2]
    arr = _lights_array(lights)
    nl = len(arr)
    name = "rt_host_reflection_chain_radiance"
    if not 1 <= S <= 64:
        raise RtError(RT_E_INVALID, f"{name}: samples {S} outside 1..64")
    if not 1 <= nl <= 16:
        raise RtError(RT_E_INVALID, f"{name}: {nl} lights, outside 1..16")
    if not 1 <= lv <= RT_MAX_REFLECTION_BOUNCES:
        raise RtError(RT_E_INVALID, f"{name}: {lv} levels, outside 1..{RT_MAX_REFLECTION_BOUNCES}")
    e = lv * n * S
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    hn = _f32(hit_normal, 4 * e)
    hg = np.ascontiguousarray(hit_group, dtype=np.uint32).ravel()
    hi = np.ascontiguousarray(hit_inst, dtype=np.uint32).ravel()
    oc = np.ascontiguousarray(occluded, dtype=np.uint8).ravel()
    va = np.ascontiguousarray(valid, dtype=np.uint8).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if hh.size != 4 * e or hg.size != e or hi.size != e or oc.size != e * nl or va.size != n or y.size != n:
        raise ValueError(f"expected {lv} x {n} x {S} records, hit groups and instances, {e * nl} occlusion bytes and "
                         f"{n} valid bytes and rows, got {hh.size // 4}, {hg.size}, {hi.size}, {oc.size}, {va.size} "
                         f"and {y.size}")
    table, _keep = _host_table(materials, instance_material)
    p = rt_reflection_chain_params(S, seed, roughness, tmax, shadow_tmin, flags, max_bounces)
    out = np.zeros((n, 4), np.float32)
    lit = np.zeros((lv, n, S, nl), np.uint8) if want_lit else None
    nrays = np.zeros((n, S), np.uint8) if want_nrays else None
    st = lib.rt_host_reflection_chain_radiance(lv, _vp(ry), _vp(hh), _vp(hn), _vp(hg), _vp(hi), _vp(oc), _vp(va),
                                               _vp(y), n, height, arr, nl, ctypes.byref(p), ctypes.byref(table),
                                               _vp(out), _vp(lit), _vp(nrays))
    if st != RT_OK:
        raise RtError(st, lib.rt_host_last_error().decode() or name)
    res = (out,) + ((lit,) if want_lit else ()) + ((nrays,) if want_nrays else ())
    return res if len(res) > 1 else out


def host_indirect_rays(cam_rays, t, normal, px, py, samples: int = 1, tmax: float = 1000.0, shadow_tmin: float = 0.01,
                       seed: int = 0, flags: int = RT_REFLECT_SHADOW_MODELS):
    """rt_host_indirect_rays: the rays rt_dispatch_indirect traces, on the host (no GPU): host_reflection_rays'
    arguments and results with the pass's directions, cosine-weighted about the facing normal (host_ao_rays'
    directions for seed `seed ^ hash(0x200)`, bit for bit). The pass's radiance twin is host_reflection_radiance_pbr
    at roughness 0 with the same samples, seed, tmax, shadow_tmin and flags."""
    cr = np.ascontiguousarray(cam_rays, dtype=np.float32).reshape(-1, 8)
    n = cr.shape[0]
    tt = _f32(t, n)
    nr = _f32(normal, 4 * n)
    x = np.ascontiguousarray(px, dtype=np.uint32).ravel()
    y = np.ascontiguousarray(py, dtype=np.uint32).ravel()
    if x.size != n or y.size != n:
        raise ValueError(f"expected {n} pixel coordinates, got {x.size} and {y.size}")
    if not 1 <= int(samples) <= 64:  # the function's own limit, checked before the output is sized by it
        raise RtError(RT_E_INVALID, f"rt_host_indirect_rays: samples {samples} outside 1..64")
    p = rt_indirect_params(samples, seed, tmax, shadow_tmin, flags)
    rays = np.zeros((n, int(samples), 8), np.float32)
    valid = np.zeros(n, np.uint8)
    st = lib.rt_host_indirect_rays(_vp(cr), _vp(tt), _vp(nr), _vp(x), _vp(y), n, ctypes.byref(p), _vp(rays),
                                   _vp(valid))
    if st != RT_OK:
        raise RtError(st, "rt_host_indirect_rays")
    return rays, valid


def host_shade_resolve_gi(width: int, height: int, camera, lights, hits, normal, object, materials,  # noqa: A002
                          instance_material=None, vis=None, ao=None, refl=None, indirect=None,
                          indirect_scale: float = 1.0, want_rgba8: bool = False):
    """rt_host_shade_resolve_gi: the PBR resolve with the indirect term on the host (no GPU). host_shade_resolve_pbr's
    arguments, and indirect: (n, 4) float32, the indirect pass's radiance plane (filtered or not), or None;
    indirect_scale: finite, >= 0. With indirect None the results are host_shade_resolve_pbr's bit for bit."""
    n = width * height
    cb = _f32(camera, 64)
    arr = _lights_array(lights)
    nl = len(arr)
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    oo = np.ascontiguousarray(object).view(np.uint32).reshape(-1)
    if hh.size != 4 * n or oo.size != 2 * n:
        raise ValueError(f"expected {4 * n} hit words and {2 * n} object words, got {hh.size} and {oo.size}")
    nn = _f32(normal, 4 * n)
    vv = None if vis is None else _f32(vis, nl * n)
    aa = None if ao is None else _f32(ao, n)
    rr = None if refl is None else _f32(refl, 4 * n)
    ii = None if indirect is None else _f32(indirect, 4 * n)
    mats, nm = _materials_array(materials)
    im = None if instance_material is None else np.ascontiguousarray(instance_material, dtype=np.uint32).ravel()
    inp = rt_resolve_gi_inputs(_vp(hh), _vp(nn), _vp(oo), _vp(vv), 0, _vp(aa), _vp(rr), _vp(ii), indirect_scale)
    table = rt_material_table(mats, nm, _vp(im), 0 if im is None else im.size)
    out = np.zeros((n, 4), np.float32)
    out8 = np.zeros((n, 4), np.uint8) if want_rgba8 else None
    st = lib.rt_host_shade_resolve_gi(width, height, _fptr(cb), arr, nl, ctypes.byref(inp), ctypes.byref(table),
                                      _vp(out), _vp(out8))
    if st != RT_OK:
        raise RtError(st, "rt_host_shade_resolve_gi")
    return (out, out8) if want_rgba8 else out


def host_reflection_composite(width: int, height: int, camera, color_in, radiance, hits, normal,
                              strength: float = 1.0, f0: float = 0.04, want_rgba8: bool = False):
    """rt_host_reflection_composite: the Fresnel composite on the host (no GPU). camera: the 64-float camera buffer;
    color_in, radiance, normal: (n, 4) float32 and hits (n, 4) uint32 (the primary G-buffer's) with n = width * height.
    Returns color (n, 4) float32 and, with want_rgba8, the (n, 4) uint8 frame as a second."""
    n = width * height
    cb = _f32(camera, 64)
    ci, rd, nn = _f32(color_in, 4 * n), _f32(radiance, 4 * n), _f32(normal, 4 * n)
    hh = np.ascontiguousarray(hits).view(np.uint32).reshape(-1)
    if hh.size != 4 * n:
        raise ValueError(f"expected {4 * n} hit words, got {hh.size}")
    p = rt_reflection_composite_params(strength, f0)
    out = np.zeros((n, 4), np.float32)
    out8 = np.zeros((n, 4), np.uint8) if want_rgba8 else None
    st = lib.rt_host_reflection_composite(width, height, _fptr(cb), ctypes.byref(p), _vp(ci), _vp(rd), _vp(hh), _vp(nn),
                                          _vp(out), _vp(out8))
    if st != RT_OK:
        raise RtError(st, "rt_host_reflection_composite")
    return (out, out8) if want_rgba8 else out


def host_denoise_guide(normal, depth):
    """rt_host_denoise_guide: the AO filter's guide plane on the host (no GPU). normal: (n, 4) G-buffer normals; depth:
    n floats, or any strided view of a float32 array (motion[:, 3]: w_cur; hits.view(float32)[:, 0]: t). Returns (n, 4)
    float32: (unit normal, depth), or four zeros where the normal is not valid or the depth is not finite and > 0."""
    nr = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1, 4)
    n = nr.shape[0]
    d = np.asarray(depth)
    if d.dtype != np.float32 or d.ndim != 1 or (n and (d.strides[0] <= 0 or d.strides[0] % 4)):
        d = np.ascontiguousarray(depth, dtype=np.float32).ravel()
    if d.size != n:
        raise ValueError(f"expected {n} depths, got {d.size}")
    out = np.zeros((n, 4), np.float32)
    st = lib.rt_host_denoise_guide(n, _vp(nr), _vp(d), d.strides[0] // 4 if n else 1, _vp(out))
    if st != RT_OK:
        raise RtError(st, "rt_host_denoise_guide")
    return out


def host_ao_accumulate(width: int, height: int, ao_cur, motion, guide_cur, ao_prev=None, hist_prev=None,
                       guide_prev=None, max_history: int = 32, depth_tol: float = 0.02, normal_cos: float = 0.9):
    """rt_host_ao_accumulate: the AO filter's temporal pass on the host (no GPU). ao_cur: width * height floats; motion,
    guide_cur: (width * height, 4); ao_prev, hist_prev, guide_prev: the previous frame's outputs and guide, or all
    None (the first frame). Returns (ao_out, hist_out), width * height float32 each."""
    n = width * height
    cur, mo, gc = _f32(ao_cur, n), _f32(motion, 4 * n), _f32(guide_cur, 4 * n)
    ap = None if ao_prev is None else _f32(ao_prev, n)
    hp = None if hist_prev is None else _f32(hist_prev, n)
    gp = None if guide_prev is None else _f32(guide_prev, 4 * n)
    p = rt_ao_temporal_params(max_history, depth_tol, normal_cos)
    ao, hist = np.zeros(n, np.float32), np.zeros(n, np.float32)
    st = lib.rt_host_ao_accumulate(width, height, ctypes.byref(p), _vp(cur), _vp(mo), _vp(gc), _vp(ap), _vp(hp),
                                   _vp(gp), _vp(ao), _vp(hist))
    if st != RT_OK:
        raise RtError(st, "rt_host_ao_accumulate")
    return ao, hist


def host_ao_atrous(width: int, height: int, ao_in, guide, iterations: int = 3, depth_tol: float = 0.02,
                   normal_cos: float = 0.9):
    """rt_host_ao_atrous: the AO filter's edge-aware a-trous blur on the host (no GPU). ao_in: width * height floats;
    guide: (width * height, 4); iterations: 1..5 (steps 1, 2, 4, 8, 16). Returns width * height float32."""
    n = width * height
    a, g = _f32(ao_in, n), _f32(guide, 4 * n)
    p = rt_ao_atrous_params(iterations, depth_tol, normal_cos)
    out, tmp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    st = lib.rt_host_ao_atrous(width, height, ctypes.byref(p), _vp(a), _vp(g), _vp(out), _vp(tmp))
    if st != RT_OK:
        raise RtError(st, "rt_host_ao_atrous")
    return out


RT_MAX_FILTER_PLANES = 17


def _host_planes(x, n: int) -> np.ndarray:
    """A plane set on the host: a 2-D array whose rows are the planes, or a sequence of them -> an own (P, n) float32
    array."""
    rows = [_f32(r, n) for r in x]
    return np.array(rows, dtype=np.float32).reshape(len(rows), n)


def _plane_table(a: np.ndarray):
    """The table of row addresses of a (P, n) array (the array must outlive the call)."""
    return (ctypes.c_void_p * a.shape[0])(*[a.ctypes.data + r * a.strides[0] for r in range(a.shape[0])])


def host_ao_accumulate_planes(width: int, height: int, cur, motion, guide_cur, prev=None, hist_prev=None,
                              guide_prev=None, max_history: int = 32, depth_tol: float = 0.02,
                              normal_cos: float = 0.9, in_place: bool = False):
    """rt_host_ao_accumulate_planes: host_ao_accumulate for P planes that share the history plane (no GPU). cur, prev:
    plane sets (a (P, width * height) array, or a sequence of planes); the other arguments as host_ao_accumulate's.
    in_place: the library is handed out[p] == cur[p] (on a copy: the caller's arrays are not written). Returns (out,
    hist_out): (P, width * height) and width * height float32."""
    n = width * height
    c, mo, gc = _host_planes(cur, n), _f32(motion, 4 * n), _f32(guide_cur, 4 * n)
    pv = None if prev is None else _host_planes(prev, n)
    if pv is not None and pv.shape[0] != c.shape[0]:
        raise ValueError(f"expected {c.shape[0]} prev planes, got {pv.shape[0]}")
    hp = None if hist_prev is None else _f32(hist_prev, n)
    gp = None if guide_prev is None else _f32(guide_prev, 4 * n)
    p = rt_ao_temporal_params(max_history, depth_tol, normal_cos)
    out = c if in_place else np.zeros_like(c)
    hist = np.zeros(n, np.float32)
    st = lib.rt_host_ao_accumulate_planes(width, height, ctypes.byref(p), c.shape[0], _plane_table(c), _vp(mo), _vp(gc),
                                          None if pv is None else _plane_table(pv), _vp(hp), _vp(gp), _plane_table(out),
                                          _vp(hist))
    if st != RT_OK:
        raise RtError(st, lib.rt_host_last_error().decode() or "rt_host_ao_accumulate_planes")
    return out, hist


def host_ao_atrous_planes(width: int, height: int, planes_in, guide, iterations: int = 3, depth_tol: float = 0.02,
                          normal_cos: float = 0.9):
    """rt_host_ao_atrous_planes: host_ao_atrous for P planes under one guide (no GPU). planes_in: a plane set, as
    host_ao_accumulate_planes'. Returns (P, width * height) float32."""
    n = width * height
    a, g = _host_planes(planes_in, n), _f32(guide, 4 * n)
    p = rt_ao_atrous_params(iterations, depth_tol, normal_cos)
    out, tmp = np.zeros_like(a), np.zeros_like(a)
    st = lib.rt_host_ao_atrous_planes(width, height, ctypes.byref(p), a.shape[0], _plane_table(a), _vp(g),
                                      _plane_table(out), _plane_table(tmp))
    if st != RT_OK:
        raise RtError(st, lib.rt_host_last_error().decode() or "rt_host_ao_atrous_planes")
    return out


def host_radiance_accumulate(width: int, height: int, rad_cur, motion, guide_cur, rad_prev=None, moments_prev=None,
                             guide_prev=None, max_history: int = 32, depth_tol: float = 0.02,
                             normal_cos: float = 0.9):
    """rt_host_radiance_accumulate: the radiance filter's temporal pass on the host (no GPU). rad_cur, motion,
    guide_cur: (width * height, 4); rad_prev, moments_prev, guide_prev: the previous frame's outputs and guide, or all
    None (the first frame). Returns (rad_out, moments_out), (width * height, 4) float32 each; a moments entry is (m1,
    m2, hist, var)."""
    n = width * height
    cur, mo, gc = _f32(rad_cur, 4 * n), _f32(motion, 4 * n), _f32(guide_cur, 4 * n)
    rp = None if rad_prev is None else _f32(rad_prev, 4 * n)
    mp = None if moments_prev is None else _f32(moments_prev, 4 * n)
    gp = None if guide_prev is None else _f32(guide_prev, 4 * n)
    p = rt_radiance_temporal_params(max_history, depth_tol, normal_cos)
    rad, mom = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    st = lib.rt_host_radiance_accumulate(width, height, ctypes.byref(p), _vp(cur), _vp(mo), _vp(gc), _vp(rp), _vp(mp),
                                         _vp(gp), _vp(rad), _vp(mom))
    if st != RT_OK:
        raise RtError(st, "rt_host_radiance_accumulate")
    return rad, mom


def host_radiance_atrous(width: int, height: int, rad_in, moments, guide, iterations: int = 3,
                         depth_tol: float = 0.02, normal_cos: float = 0.9, sigma_l: float = 4.0):
    """rt_host_radiance_atrous: the radiance filter's variance-guided a-trous blur on the host (no GPU). rad_in,
    moments, guide: (width * height, 4); only moments[:, 3], the variance, is read. Returns (rad_out (width * height,
    4), var_out width * height) float32."""
    n = width * height
    a, m, g = _f32(rad_in, 4 * n), _f32(moments, 4 * n), _f32(guide, 4 * n)
    p = rt_radiance_atrous_params(iterations, depth_tol, normal_cos, sigma_l)
    out, tmp = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    var, vtmp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    st = lib.rt_host_radiance_atrous(width, height, ctypes.byref(p), _vp(a), _vp(m), _vp(g), _vp(out), _vp(var),
                                     _vp(tmp), _vp(vtmp))
    if st != RT_OK:
        raise RtError(st, "rt_host_radiance_atrous")
    return out, var


def host_reflection_motion(width: int, height: int, hits, guide_cur, motion, dist, camera, prev_camera,
                           guide_prev=None, share: float = 1.0, static_tol: float = REFLECTION_MOTION_STATIC_TOL,
                           depth_tol: float = 0.02, normal_cos: float = 0.9):
    """rt_host_reflection_motion: the reflection motion plane on the host (no GPU). hits: (width * height, 4) 32-bit
    words (dispatch_gbuffer's hits); guide_cur, motion: (width * height, 4) floats; dist: width * height floats, or any
    strided view of a float32 array (rad[:, 3]: a reflection plane's distance); camera / prev_camera: the two frames'
    64-float camera buffers; guide_prev: the previous frame's guide or None (class 6 is then not evaluated). Returns
    (motion_out (width * height, 4) float32, classes width * height uint8: 0 virtual, 1..6 the pass-through classes of
    include/rt_api.h). static_tol's default, 2^-4 px, is 16 x the largest distance measured between the static point's
    entry and the motion plane's on static geometry (0.00256 px, C2F at 1080p), rounded up to a power of two (DESIGN
    §3.19)."""
    n = width * height
    hw = np.ascontiguousarray(hits)
    if hw.dtype.itemsize != 4 or hw.size != 4 * n:
        raise ValueError(f"expected {4 * n} 32-bit hit words, got {hw.size} of {hw.dtype.itemsize} bytes")
    gc, mo = _f32(guide_cur, 4 * n), _f32(motion, 4 * n)
    d = np.asarray(dist)
    if d.dtype != np.float32 or d.ndim != 1 or (n and (d.strides[0] <= 0 or d.strides[0] % 4)):
        d = np.ascontiguousarray(dist, dtype=np.float32).ravel()
    if d.size != n:
        raise ValueError(f"expected {n} distances, got {d.size}")
    gp = None if guide_prev is None else _f32(guide_prev, 4 * n)
    cb = None if camera is None else _f32(camera, 64)
    pcb = None if prev_camera is None else _f32(prev_camera, 64)
    p = rt_reflection_motion_params(share, static_tol, depth_tol, normal_cos)
    out, cls = np.zeros((n, 4), np.float32), np.zeros(n, np.uint8)
    st = lib.rt_host_reflection_motion(width, height, ctypes.byref(p), _vp(hw), _vp(gc), _vp(mo), _vp(d),
                                       d.strides[0] // 4 if n else 1, _vp(gp), _vp(cb), _vp(pcb), _vp(out), _vp(cls))
    if st != RT_OK:
        raise RtError(st, "rt_host_reflection_motion")
    return out, cls


def _upscale_params(jitter_cur, jitter_prev, max_history, depth_tol) -> rt_upscale_params:
    jc, jp = _f32(jitter_cur, 2), _f32(jitter_prev, 2)
    return rt_upscale_params((ctypes.c_float * 2)(*jc.tolist()), (ctypes.c_float * 2)(*jp.tolist()), max_history,
                             depth_tol)


def host_upscale(render_width: int, render_height: int, width: int, height: int, color_cur, motion_cur,
                 motion_prev=None, color_prev=None, hist_prev=None, jitter_cur=(0.0, 0.0), jitter_prev=(0.0, 0.0),
                 max_history: int = 16, depth_tol: float = 0.02, want_rgba8: bool = False):
    """rt_host_upscale: the temporal upscaler on the host (no GPU). color_cur, motion_cur: (render_width *
    render_height, 4); motion_prev likewise, color_prev (width * height, 4) and hist_prev (width * height): the previous
    frame's motion plane and outputs, or all None (the first frame). Returns (color_out (width * height, 4), hist_out
    (width * height)) and, with want_rgba8, the (width * height, 4) uint8 frame as a third."""
    n, N = render_width * render_height, width * height
    cc, mc = _f32(color_cur, 4 * n), _f32(motion_cur, 4 * n)
    mp = None if motion_prev is None else _f32(motion_prev, 4 * n)
    cp = None if color_prev is None else _f32(color_prev, 4 * N)
    hp = None if hist_prev is None else _f32(hist_prev, N)
    p = _upscale_params(jitter_cur, jitter_prev, max_history, depth_tol)
    out, hist = np.zeros((N, 4), np.float32), np.zeros(N, np.float32)
    out8 = np.zeros((N, 4), np.uint8) if want_rgba8 else None
    st = lib.rt_host_upscale(render_width, render_height, width, height, ctypes.byref(p), _vp(cc), _vp(mc), _vp(mp),
                             _vp(cp), _vp(hp), _vp(out), _vp(hist), _vp(out8))
    if st != RT_OK:
        raise RtError(st, "rt_host_upscale")
    return (out, hist, out8) if want_rgba8 else (out, hist)


def camera_jitter(camera, width: int, height: int, jx: float, jy: float) -> np.ndarray:
    """rt_camera_jitter: the 64-float camera buffer whose pixel-centre rays are `camera`'s rays through (px + 0.5 + jx,
    py + 0.5 + jy) of a width x height frame, and whose forward projection lands at (x - jx, y - jy). |j| < 0.5."""
    cb = _f32(camera, 64)
    out = np.zeros(64, np.float32)
    st = lib.rt_camera_jitter(_fptr(cb), width, height, jx, jy, _fptr(out))
    if st != RT_OK:
        raise RtError(st, "rt_camera_jitter")
    return out


def jitter_halton(index: int):
    """rt_jitter_halton: element 1 + index % (3^15 - 1) of the Halton sequence in bases (2, 3), minus 0.5: a jitter
    (jx, jy) for camera_jitter, as two Python floats holding float32 values."""
    out = np.zeros(2, np.float32)
    st = lib.rt_jitter_halton(index, _fptr(out))
    if st != RT_OK:
        raise RtError(st, "rt_jitter_halton")
    return float(out[0]), float(out[1])


class Manipulator:
    """Camera manipulator with the reference's API (nv_helpers_dx12::Manipulator,
    include/manipulator.h:33-148, src/manipulator.cpp) over the C-ABI rt_manip_* functions.
    Host-only arithmetic; results are bit-identical to the reference's glm arithmetic."""
    Examine, Fly, Walk, Trackball = 0, 1, 2, 3          # Modes, manipulator.h:37
    NoAction, Orbit, Dolly, Pan, LookAround = 0, 1, 2, 3, 4  # Actions, manipulator.h:38
    LMB, MMB, RMB, SHIFT, CTRL, ALT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20  # Inputs bits

    def __init__(self):
        self._m = rt_manipulator()
        lib.rt_manip_init(ctypes.byref(self._m))

    @staticmethod
    def inputs(lmb=False, mmb=False, rmb=False, shift=False, ctrl=False, alt=False) -> int:
        """Manipulator::Inputs (manipulator.h:39-40) -> RT_INPUT_* bits."""
        return (lmb * 0x01) | (mmb * 0x02) | (rmb * 0x04) | (shift * 0x08) | (ctrl * 0x10) | (alt * 0x20)

    def setLookat(self, eye, center, up):
        e, c, u = _f32(eye, 3), _f32(center, 3), _f32(up, 3)
        lib.rt_manip_set_lookat(ctypes.byref(self._m), _fptr(e), _fptr(c), _fptr(u))

    def getLookat(self):
        m = self._m
        return (np.array(m.pos[:], np.float32), np.array(m.interest[:], np.float32), np.array(m.up[:], np.float32))

    def setWindowSize(self, w: int, h: int):
        lib.rt_manip_set_window_size(ctypes.byref(self._m), w, h)

    def getWidth(self) -> int:
        return self._m.width

    def getHeight(self) -> int:
        return self._m.height

    def setMousePosition(self, x: int, y: int):
        lib.rt_manip_set_mouse_position(ctypes.byref(self._m), x, y)

    def getMousePosition(self):
        return int(self._m.mouse[0]), int(self._m.mouse[1])

    def setMode(self, mode: int):
        self._m.mode = mode

    def getMode(self) -> int:
        return self._m.mode

    def setRoll(self, roll: float):
        lib.rt_manip_set_roll(ctypes.byref(self._m), roll)

    def getRoll(self) -> float:
        return self._m.roll

    def setSpeed(self, speed: float):
        self._m.speed = speed

    def getSpeed(self) -> float:
        return self._m.speed

    def getMatrix(self) -> np.ndarray:
        """Column-major 4x4 as glm stores it (16 floats)."""
        return np.array(self._m.matrix[:], np.float32)

    def motion(self, x: int, y: int, action: int = 0):
        lib.rt_manip_motion(ctypes.byref(self._m), x, y, action)

    def mouseMove(self, x: int, y: int, inputs: int) -> int:
        return int(lib.rt_manip_mouse_move(ctypes.byref(self._m), x, y, inputs))

    def wheel(self, value: int):
        lib.rt_manip_wheel(ctypes.byref(self._m), value)


def strip_rows(height: int, nranks: int, rank: int, strip_rows_: int = 8) -> np.ndarray:
    n = lib.rt_strip_rows(height, nranks, rank, strip_rows_, None, 0)
    out = np.zeros(n, np.uint32)
    lib.rt_strip_rows(height, nranks, rank, strip_rows_, out.ctypes.data_as(_P), n)
    return out


class PipelineEvent:
    """rt_event_*: a device-side sync point between the strips loop's render and gather streams
    (no timestamp, no system-scope fence on record). record(stream) / wait_on(stream) take raw
    hipStream_t handles (torch: stream.cuda_stream)."""

    def __init__(self):
        h = _P()
        st = lib.rt_event_create(ctypes.byref(h))
        if st != RT_OK:
            raise RtError(st, "rt_event_create")
        self._h = h

    def record(self, stream: Optional[int]):
        st = lib.rt_event_record(self._h, stream)
        if st != RT_OK:
            raise RtError(st, "rt_event_record")

    def wait_on(self, stream: Optional[int]):
        """Later work on `stream` waits for this event's last record."""
        st = lib.rt_stream_wait_event(stream, self._h)
        if st != RT_OK:
            raise RtError(st, "rt_stream_wait_event")

    def close(self):
        if self._h:
            lib.rt_event_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


RT_COMM_ID_BYTES = 128


def comm_available() -> bool:
    """rt_comm_available: RCCL can be loaded (no collective, no GPU work)."""
    return lib.rt_comm_available() == RT_OK


def comm_unique_id() -> bytes:
    """rt_comm_get_unique_id (ncclGetUniqueId): created on rank 0, handed to every rank by the caller."""
    buf = ctypes.create_string_buffer(RT_COMM_ID_BYTES)
    st = lib.rt_comm_get_unique_id(buf)
    if st != RT_OK:
        raise RtError(st, "rt_comm_get_unique_id")
    return buf.raw


class Comm:
    """rt_comm_*: the native multi-GPU frame loop (strips -> ncclGather -> assembly on rank 0) of one context.
    Collective: every rank constructs it with the same 128-byte id and calls render_strips in the same order."""

    def __init__(self, ctx: "Context", nranks: int, rank: int, uid: Optional[bytes]):
        """uid None: a loopback communicator (rt_comm_init_loopback, tests): this process renders every one of
        the nranks ranks on its one GPU and the gather is a device copy (rank must be 0)."""
        self._lib = ctx._lib
        self.ctx, self.nranks, self.rank = ctx, nranks, rank
        self.is_loopback = uid is None
        self._pending = False  # frames handed to render_strips* since the last synchronize (a partly filled batch)
        h = _P()
        if uid is None:
            if rank != 0:
                raise ValueError("a loopback communicator is rank 0")
            st = self._lib.rt_comm_init_loopback(ctx._h, nranks, ctypes.byref(h))
            if st != RT_OK:
                raise RtError(st, f"rt_comm_init_loopback(nranks={nranks})")
            self._h = h
            return
        if len(uid) != RT_COMM_ID_BYTES:
            raise ValueError("the communicator id is 128 bytes")
        self._idbuf = ctypes.create_string_buffer(uid, RT_COMM_ID_BYTES)
        st = self._lib.rt_comm_init(ctx._h, nranks, rank, self._idbuf, ctypes.byref(h))
        if st != RT_OK:
            raise RtError(st, f"rt_comm_init(nranks={nranks}, rank={rank})")
        self._h = h

    @classmethod
    def loopback(cls, ctx: "Context", nranks: int) -> "Comm":
        """rt_comm_init_loopback: nranks ranks emulated by this process on its one GPU (no RCCL)."""
        return cls(ctx, nranks, 0, None)

    def _check(self, st: int, what: str):
        if st != RT_OK:
            raise RtError(st, f"{what}: {self._lib.rt_comm_last_error(self._h).decode()}")

    def render_strips(self, width: int, height: int, frame_out=None, stream: Optional[int] = None,
                      strip_rows_: int = 8):
        """One tiled frame (rt_render_strips): frame_out is rank 0's H x W x 4 device buffer."""
        self._pending = True
        self._check(self._lib.rt_render_strips(self._h, width, height, strip_rows_, _ptr(frame_out), stream),
                    "rt_render_strips")

    def render_strips_frames(self, width: int, height: int, frames_out, cameras=None, stream: Optional[int] = None,
                             strip_rows_: int = 8):
        """rt_render_strips_frames: len(frames_out) frames in one launch per rank (cameras: n x 64 floats or None =
        the context's camera); frames_out: rank 0's device buffers (None entries on other ranks)."""
        n = len(frames_out)
        ptrs = (_P * n)(*[_ptr(f) for f in frames_out])
        cams = None if cameras is None else _f32(cameras, 64 * n)
        self._pending = True
        self._check(self._lib.rt_render_strips_frames(self._h, width, height, strip_rows_, n,
                                                      None if cams is None else _fptr(cams), ptrs, stream),
                    "rt_render_strips_frames")

    @property
    def stream(self) -> int:
        """hipStream_t of the gathers, made to wait for every step issued so far (rt_comm_stream)."""
        return self._lib.rt_comm_stream(self._h)

    @property
    def depth(self) -> int:
        """Frames in the pipeline: slots (one render stream each) x frames per gather; a caller that gives each
        call its own frame buffer needs this many to never wait on a frame buffer's previous assembly."""
        return int(self._lib.rt_comm_pipeline_depth(self._h))

    def set_batch(self, frames_per_gather: int):
        """rt_comm_set_batch: frames whose strips go in one ncclGather (every rank the same, between the same calls)."""
        self._check(self._lib.rt_comm_set_batch(self._h, frames_per_gather), "rt_comm_set_batch")

    @property
    def batch(self) -> int:
        return int(self._lib.rt_comm_batch(self._h))

    def synchronize(self):
        self._check(self._lib.rt_comm_synchronize(self._h), "rt_comm_synchronize")
        self._pending = False

    def close(self):
        """rt_comm_destroy: drains the pipeline (a partly filled batch included), then frees the communicator.
        Collective for an RCCL communicator: EVERY rank must call close() (or every rank abort()); a rank that drops
        its communicator unclosed aborts it (__del__), and a peer draining a partly filled batch would then wait for
        a gather that rank never issues."""
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            st = self._lib.rt_comm_destroy(h)
            if st != RT_OK:
                raise RtError(st, "rt_comm_destroy")

    def set_phase_timing(self, on: bool):
        """rt_comm_set_phase_timing: timing-event pairs around each step's render, gather and assembly (drains)."""
        self._check(self._lib.rt_comm_set_phase_timing(self._h, 1 if on else 0), "rt_comm_set_phase_timing")
        self._pending = False

    def phase_stats(self) -> dict:
        """rt_comm_phase_stats: the phase sums since set_phase_timing(True) (drains the pipeline)."""
        out = (ctypes.c_double * 12)()
        self._check(self._lib.rt_comm_phase_stats(self._h, out, 12), "rt_comm_phase_stats")
        self._pending = False
        return dict(zip(("frames", "renders", "render_ms", "gathers", "gather_ms", "assemblies", "assembly_ms",
                         "host_us", "calls", "issue_us", "bytes_in", "bytes"), list(out)))

    def loopback_render_ranks(self, first: int = 0, count: int = 0):
        """rt_comm_loopback_render_ranks: a loopback communicator renders only emulated ranks [first, first + count)
        (0: all) — the rehearsal of one rank's share of a step; the other ranks' strips are stale."""
        self._check(self._lib.rt_comm_loopback_render_ranks(self._h, first, count), "rt_comm_loopback_render_ranks")

    def abort(self):
        """rt_comm_abort: the failure path. Frees the communicator without another collective (the partly filled
        batch is discarded, ncclCommAbort cancels gathers in flight): safe when other ranks may never call again."""
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            st = self._lib.rt_comm_abort(h)
            if st != RT_OK:
                raise RtError(st, "rt_comm_abort")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        # a normal exit drains (collective); an exception may have left the ranks out of step: abort
        if exc_type is None:
            self.close()
        else:
            self.abort()
        return False

    def __del__(self):
        # An unclosed communicator is garbage. Loopback: no peers, so it drains like close() (frames already handed
        # to render_strips are rendered and assembled). RCCL: the other ranks may not issue the collective a
        # draining destroy would need (an exception path, interpreter shutdown), so it aborts -- and says so when
        # that discards frames (close() is required on every rank).
        if not getattr(self, "_h", None):
            return
        try:
            if self.is_loopback:
                self.close()
                return
            if self._pending:
                import warnings
                warnings.warn("rt.Comm garbage-collected unclosed with frames pending: aborted (their partly filled "
                              "batch is discarded); call close() on every rank", ResourceWarning, stacklevel=2)
            self.abort()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def strip_rows_per_rank(height: int, nranks: int, strip_rows_: int = 8) -> int:
    """Rows of the padded per-rank buffer that rt_assemble_strips expects (rank-major blocks)."""
    nstrips = (height + strip_rows_ - 1) // strip_rows_
    return ((nstrips + nranks - 1) // nranks) * strip_rows_


# ---------------------------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------------------------

def _ptr(x) -> Optional[int]:
    """Device pointer of a torch tensor, an int address, or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return x.data_ptr()


class Context:
    """One rt_ctx (one HIP device, one host thread)."""

    def __init__(self, device: int = 0, library: Optional[ctypes.CDLL] = None):
        self._lib = library if library is not None else lib
        h = _P()
        st = self._lib.rt_create(device, ctypes.byref(h))
        if st != RT_OK:
            raise RtError(st, f"rt_create(device={device})")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self._lib.rt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st: int, what: str):
        if st != RT_OK:
            raise RtError(st, f"{what}: {self._lib.rt_last_error(self._h).decode()}")

    # acceleration structures ------------------------------------------------------------------
    def blas_build(self, vertices: np.ndarray, indices: Optional[np.ndarray] = None) -> int:
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        stride = v.shape[1] * 4 if v.ndim == 2 else 24
        nv = v.shape[0] if v.ndim == 2 else v.size // 6
        out = _U32()
        if indices is None:
            st = self._lib.rt_blas_build(self._h, v.ctypes.data_as(_P), nv, stride, None, 0, ctypes.byref(out))
        else:
            i = np.ascontiguousarray(indices, dtype=np.uint32)
            st = self._lib.rt_blas_build(self._h, v.ctypes.data_as(_P), nv, stride, i.ctypes.data_as(_P), i.size,
                                   ctypes.byref(out))
        self._check(st, "rt_blas_build")
        return out.value

    def blas_rebuild(self, blas: int, vertices: np.ndarray, indices: Optional[np.ndarray] = None):
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        stride = v.shape[1] * 4
        if indices is None:
            st = self._lib.rt_blas_rebuild(self._h, blas, v.ctypes.data_as(_P), v.shape[0], stride, None, 0)
        else:
            i = np.ascontiguousarray(indices, dtype=np.uint32)
            st = self._lib.rt_blas_rebuild(self._h, blas, v.ctypes.data_as(_P), v.shape[0], stride,
                                     i.ctypes.data_as(_P), i.size)
        self._check(st, "rt_blas_rebuild")

    def blas_refit(self, blas: int, vertices: np.ndarray):
        """rt_blas_refit: new vertices for the BLAS's topology, boxes refitted in place. vertices: (vcount, k)
        floats, k >= 6 replaces positions and normals, 3 <= k < 6 the positions only. tlas_build (update_only
        allowed) must follow before the next launch."""
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        if v.ndim != 2:
            v = v.reshape(-1, 6)
        self._check(self._lib.rt_blas_refit(self._h, blas, v.ctypes.data_as(_P), v.shape[0], v.shape[1] * 4),
                    "rt_blas_refit")

    def blas_refit_device(self, blas: int, tensor, stream: Optional[int] = None):
        """rt_blas_refit_device: as blas_refit from a contiguous float32 device tensor of shape (vcount, 3) or
        (vcount, 6), read after the work already enqueued on `stream` (a raw hipStream_t; None: the default)."""
        if tensor.dim() != 2 or tensor.shape[1] not in (3, 6) or not tensor.is_contiguous() \
                or tensor.dtype != torch.float32 or not tensor.is_cuda:
            raise ValueError("blas_refit_device: a contiguous float32 device tensor of shape (vcount, 3 | 6)")
        self._check(self._lib.rt_blas_refit_device(self._h, blas, tensor.data_ptr(), int(tensor.shape[0]),
                                                   int(tensor.shape[1]) * 4, stream), "rt_blas_refit_device")

    def blas_info(self, blas: int) -> rt_bvh_info:
        info = rt_bvh_info()
        self._check(self._lib.rt_blas_info(self._h, blas, ctypes.byref(info)), "rt_blas_info")
        return info

    def blas_export(self, blas: int):
        info = self.blas_info(blas)
        nodes = np.zeros(info.node_count * 32, np.uint32)  # 128-B 4-wide nodes
        tris = np.zeros(info.prim_count * 12, np.uint32)
        self._check(self._lib.rt_blas_export(self._h, blas, nodes.ctypes.data_as(_P), nodes.nbytes,
                                             tris.ctypes.data_as(_P), tris.nbytes), "rt_blas_export")
        return nodes.reshape(-1, 32), tris.reshape(-1, 12)

    def tlas_build(self, instances: Sequence[tuple], update_only: bool = False):
        """instances: (blas, xform3x4 (12 floats), instance_id, hit_group) tuples."""
        arr = (rt_instance * len(instances))()
        for k, (b, x, iid, hg) in enumerate(instances):
            arr[k].blas = b
            arr[k].xform3x4_rowmajor[:] = [float(v) for v in np.asarray(x, np.float32).ravel()]
            arr[k].instance_id = iid
            arr[k].hit_group = hg
        self._check(self._lib.rt_tlas_build(self._h, arr, len(instances), 1 if update_only else 0), "rt_tlas_build")

    def tlas_info(self) -> rt_bvh_info:
        info = rt_bvh_info()
        self._check(self._lib.rt_tlas_info(self._h, ctypes.byref(info)), "rt_tlas_info")
        return info

    def tlas_build_wall_ms(self) -> float:
        """Host wall time of the last tlas_build (ms)."""
        return float(self._lib.rt_tlas_build_wall_ms(self._h))

    def tlas_export(self) -> np.ndarray:
        info = self.tlas_info()
        nodes = np.zeros(info.node_count * 32, np.uint32)
        self._check(self._lib.rt_tlas_export(self._h, nodes.ctypes.data_as(_P), nodes.nbytes), "rt_tlas_export")
        return nodes.reshape(-1, 32)

    # frame state ------------------------------------------------------------------------------
    def set_camera(self, cb: np.ndarray):
        c = _f32(cb, 64)
        self._check(self._lib.rt_set_camera(self._h, _fptr(c)), "rt_set_camera")

    def set_shading(self, lights: Iterable, material, mode: int, spp: int = 1):
        lights = list(lights)
        arr = (rt_light * len(lights))()
        for k, (col, pos, inten) in enumerate(lights):
            arr[k].color[:] = [float(v) for v in col]
            arr[k].position[:] = [float(v) for v in pos]
            arr[k].intensity = float(inten)
        m = rt_material()
        m.albedo[:] = [float(v) for v in material[0:3]]
        m.roughness, m.metallic, m.reflectivity = (float(v) for v in material[3:6])
        self._check(self._lib.rt_set_shading(self._h, arr, len(lights), ctypes.byref(m), mode, spp), "rt_set_shading")
        self._nlights = len(lights)  # the visibility planes' count (dispatch_shadow, shade_resolve size their tensors)

    def set_schedule(self, schedule: int):
        self._check(self._lib.rt_set_schedule(self._h, schedule), "rt_set_schedule")

    def set_triangle_test(self, mode: int):
        """rt_set_triangle_test: RT_TRIANGLE_TEST_MOLLER_TRUMBORE (default) or RT_TRIANGLE_TEST_WATERTIGHT."""
        self._check(self._lib.rt_set_triangle_test(self._h, mode), "rt_set_triangle_test")

    def set_tile_rows(self, rows: int):
        """rt_set_tile_rows: 8 (8 x 8 pixel tiles per wave, default) or 4 (8 x 4)."""
        self._check(self._lib.rt_set_tile_rows(self._h, rows), "rt_set_tile_rows")

    def set_tile_balance(self, mode: int):
        """rt_set_tile_balance: 0 off, 1 adaptive (default), 2 / 3 / 4 / 5 forced split layouts (tests)."""
        self._check(self._lib.rt_set_tile_balance(self._h, mode), "rt_set_tile_balance")

    def tile_balance_info(self) -> dict:
        out = (ctypes.c_uint32 * RT_BALANCE_INFO_COUNT)()
        self._check(self._lib.rt_tile_balance_info_n(self._h, out, RT_BALANCE_INFO_COUNT), "rt_tile_balance_info_n")
        return dict(zip(("plans", "split", "items", "extra_cap", "max_ticks", "mean_ticks", "threshold", "launches",
                         "pays", "check_bad", "check_first_tile", "check_first_word", "plan_load_ticks",
                         "plan_budget_ticks", "plan_place_ticks", "slots", "refused", "refused_plans"), list(out)))

    def counters(self) -> dict:
        """rt_ctx_counters_n: device-wide synchronisations, tile-balance maps recycled / full, maps held, recycled maps
        that reached a plan."""
        out = (ctypes.c_uint64 * 5)()
        self._check(self._lib.rt_ctx_counters_n(self._h, out, 5), "rt_ctx_counters_n")
        return dict(zip(("device_syncs", "balance_recycled", "balance_full", "balance_maps", "balance_recycled_planned"),
                        list(out)))

    def tile_plan_probe(self, costs, **knobs):
        """rt_tile_plan_probe (diagnostics): the plan kernel once on `costs` (2 * ntiles words) with rt_tile_plan_args'
        knobs as keywords. Returns (the list as stored: uint32 array, the summary: dict, the costs as the plan left
        them: uint32 array)."""
        a = rt_tile_plan_args(**knobs)
        cost = np.ascontiguousarray(costs, dtype=np.uint32)
        if cost.size != 2 * a.ntiles:
            raise ValueError("tile_plan_probe: costs must hold 2 * ntiles words")
        groups = -(-(a.ntiles + a.extra_cap) // max(1, a.wl))
        plan = np.zeros(1 + -(-groups // 8) * 8 * a.wl, dtype=np.uint32)
        stats = np.zeros(RT_TILE_PLAN_STATS, dtype=np.uint32)
        left = np.zeros_like(cost)
        self._check(self._lib.rt_tile_plan_probe(self._h, ctypes.byref(a), cost.ctypes.data_as(_UP),
                                                 plan.ctypes.data_as(_UP), plan.size, stats.ctypes.data_as(_UP),
                                                 stats.size, left.ctypes.data_as(_UP)), "rt_tile_plan_probe")
        return plan, dict(zip(TILE_PLAN_STAT_NAMES, (int(x) for x in stats))), left

    def set_stats(self, on: bool):
        self._check(self._lib.rt_set_stats(self._h, 1 if on else 0), "rt_set_stats")

    def stats(self) -> dict:
        out = (ctypes.c_uint64 * len(STAT_NAMES))()
        self._check(self._lib.rt_stats(self._h, out), "rt_stats")
        return dict(zip(STAT_NAMES, list(out)))

    def stats_reset(self):
        self._check(self._lib.rt_stats_reset(self._h), "rt_stats_reset")

    # launches ---------------------------------------------------------------------------------
    @staticmethod
    def _rows_arg(rows, height: int):
        """A launch's rows argument as (pointer, count, the array that owns the pointer: kept until the call returns);
        None: every row of the frame."""
        if rows is None:
            return None, height, None
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        return r.ctypes.data_as(_P), r.size, r

    @staticmethod
    def _set_planes(g, method: str, entries: int, planes):
        """Fills the output structure g from planes, (name, tensor or address or None, 32-bit words per entry) each: a
        tensor must hold exactly `entries` entries."""
        for name, t, words in planes:
            if t is not None and not isinstance(t, int):
                if t.element_size() != 4 or t.numel() != entries * words or not t.is_contiguous():
                    raise ValueError(f"{method}: {name} must be a contiguous tensor of {entries * words} "
                                     f"32-bit elements, got {t.numel()} of {t.element_size()} bytes")
            setattr(g, name, _ptr(t))

    def dispatch(self, width: int, height: int, rgba8, rgba32f=None, rows: Optional[np.ndarray] = None,
                 stream: Optional[int] = None):
        rp, nr, _keep = self._rows_arg(rows, height)
        self._check(self._lib.rt_dispatch_rays(self._h, width, height, rp, nr, _ptr(rgba8), _ptr(rgba32f), stream),
                    "rt_dispatch_rays")

    def dispatch_frames(self, width: int, height: int, rgba8, cameras=None, stream: Optional[int] = None,
                        frame_stride: int = 0):
        """rt_dispatch_frames: len(rgba8) (1..4) full frames in one launch. rgba8: an (n, H, W, 4) uint8 device
        tensor (frames back to back, or frame_stride bytes apart); cameras: n x 64 floats (None: the context's
        camera for every frame)."""
        n = int(rgba8.shape[0])
        cams = None if cameras is None else _f32(cameras, 64 * n)
        self._pending = True
        self._check(self._lib.rt_dispatch_frames(self._h, width, height, n, None if cams is None else _fptr(cams),
                                                 _ptr(rgba8), frame_stride, stream), "rt_dispatch_frames")

    def dispatch_gbuffer(self, width: int, height: int, hits=None, uv=None, normal=None, object=None,  # noqa: A002
                         rows: Optional[np.ndarray] = None, stream: Optional[int] = None):
        """rt_dispatch_gbuffer: the frame's primary-visibility planes, nrows * width entries each in the compact row
        order of dispatch(): hits (4 x 32-bit words per pixel: t, instance id, primitive, hit flag), uv (2 floats),
        normal (4 floats, w = 0), object (2 words: instance index, hit group). Device tensors (or raw addresses); a
        plane left None is not written; at least one must be given."""
        rp, nr, _keep = self._rows_arg(rows, height)
        g = rt_gbuffer()
        self._set_planes(g, "dispatch_gbuffer", nr * width,
                         (("hits", hits, 4), ("uv", uv, 2), ("normal", normal, 4), ("object", object, 2)))
        self._check(self._lib.rt_dispatch_gbuffer(self._h, width, height, rp, nr, ctypes.byref(g), stream),
                    "rt_dispatch_gbuffer")

    def set_motion_history(self, on: bool):
        """rt_set_motion_history: from the next tlas_build on, each TLAS version keeps every instance's previous
        transform and its BLAS's positions before the interval's first refit (dispatch_gbuffer_motion's inputs)."""
        self._check(self._lib.rt_set_motion_history(self._h, 1 if on else 0), "rt_set_motion_history")

    def dispatch_gbuffer_motion(self, width: int, height: int, hits=None, uv=None, normal=None, object=None,  # noqa: A002
                                motion=None, prev_camera=None, rows: Optional[np.ndarray] = None,
                                stream: Optional[int] = None):
        """rt_dispatch_gbuffer_motion: dispatch_gbuffer's planes and motion (4 floats per pixel: mx, my, w_prev,
        w_cur — the pixel's surface point was at (x + 0.5 + mx, y + 0.5 + my) in the previous frame, +inf when it was
        behind the previous camera; the two view depths). prev_camera: the previous frame's 64-float camera buffer
        (None: the current camera). motion needs set_motion_history(True) before the TLAS was built."""
        rp, nr, _keep = self._rows_arg(rows, height)
        g = rt_gbuffer_motion()
        self._set_planes(g, "dispatch_gbuffer_motion", nr * width,
                         (("hits", hits, 4), ("uv", uv, 2), ("normal", normal, 4), ("object", object, 2),
                          ("motion", motion, 4)))
        pcb = None if prev_camera is None else _f32(prev_camera, 64)
        self._check(self._lib.rt_dispatch_gbuffer_motion(self._h, width, height, rp, nr, ctypes.byref(g),
                                                         None if pcb is None else _fptr(pcb), stream),
                    "rt_dispatch_gbuffer_motion")

    def dispatch_with_gbuffer(self, width: int, height: int, rgba8, rgba32f=None, hits=None, uv=None, normal=None,
                              object=None, motion=None, prev_camera=None,  # noqa: A002
                              rows: Optional[np.ndarray] = None, stream: Optional[int] = None):
        """rt_dispatch_rays_gbuffer: dispatch() and dispatch_gbuffer_motion() in one launch with one primary walk per
        pixel. rgba8 / rgba32f come out as dispatch() writes them, the planes as dispatch_gbuffer_motion() does, bit for
        bit. One sample per pixel only (set_shading's spp must be 1); always the plain grid (set_tile_balance and
        set_tile_rows do not apply); at least one plane must be given."""
        rp, nr, _keep = self._rows_arg(rows, height)
        g = rt_gbuffer_motion()
        self._set_planes(g, "dispatch_with_gbuffer", nr * width,
                         (("hits", hits, 4), ("uv", uv, 2), ("normal", normal, 4), ("object", object, 2),
                          ("motion", motion, 4)))
        pcb = None if prev_camera is None else _f32(prev_camera, 64)
        self._check(self._lib.rt_dispatch_rays_gbuffer(self._h, width, height, rp, nr, _ptr(rgba8), _ptr(rgba32f),
                                                       ctypes.byref(g), None if pcb is None else _fptr(pcb), stream),
                    "rt_dispatch_rays_gbuffer")

    def dispatch_ao(self, width: int, height: int, ao, samples: int, radius: float, tmin: float = 0.01, seed: int = 0,
                    rows: Optional[np.ndarray] = None, stream: Optional[int] = None):
        """rt_dispatch_ao: ambient occlusion of the frame dispatch_gbuffer describes, one float per pixel (nrows *
        width entries in dispatch()'s compact row order; a device tensor or a raw address): the share of `samples`
        (1..64) cosine-weighted rays from the primary hit over [tmin, radius] that hit nothing; 1.0 on a miss. The
        same seed gives the same plane bit for bit; host_ao_rays gives the rays."""
        rp, nr, _keep = self._rows_arg(rows, height)
        if ao is not None and not isinstance(ao, int):
            if ao.element_size() != 4 or ao.numel() != nr * width or not ao.is_contiguous():
                raise ValueError(f"dispatch_ao: ao must be a contiguous tensor of {nr * width} 32-bit elements, got "
                                 f"{ao.numel()} of {ao.element_size()} bytes")
        p = rt_ao_params(samples, seed, radius, tmin)
        self._check(self._lib.rt_dispatch_ao(self._h, width, height, rp, nr, ctypes.byref(p), _ptr(ao), stream),
                    "rt_dispatch_ao")

    def _vis_planes(self, method: str, vis, entries: int, stride: int, nlights: Optional[int]):
        """Checks a tensor of visibility planes: `nlights` planes (None: the count Context.set_shading was last given)
        of `entries` floats, `stride` floats apart (0: back to back), must fit in it. The library cannot check a
        tensor's size, so a context whose lights were set some other way (the raw library) must say how many there
        are. A stride below `entries` is left to the library to refuse; a raw address is not checked."""
        if vis is None or isinstance(vis, int):
            return
        nl = getattr(self, "_nlights", None) if nlights is None else int(nlights)
        if nl is None:
            raise ValueError(f"{method}: the light count is not known to this Context (set_shading was not called "
                             f"through it): pass nlights, so that the planes' tensor can be checked")
        need = (nl - 1) * max(stride or entries, entries) + entries
        if vis.element_size() != 4 or not vis.is_contiguous() or vis.numel() < need:
            raise ValueError(f"{method}: vis must be a contiguous tensor of at least {need} 32-bit elements ({nl} "
                             f"planes of {entries}), got {vis.numel()} of {vis.element_size()} bytes")

    def dispatch_shadow(self, width: int, height: int, vis, samples: int = 1, light_radius: float = 0.0,
                        tmin: float = 0.01, seed: int = 0, rows: Optional[np.ndarray] = None, plane_stride: int = 0,
                        stream: Optional[int] = None, nlights: Optional[int] = None):
        """rt_dispatch_shadow: per light of set_shading a visibility plane of the frame dispatch_gbuffer describes, one
        float per pixel (nrows * width entries in dispatch()'s compact row order): the share of `samples` (1..64)
        any-hit rays from the primary hit towards the light's sphere (radius light_radius; 0: its centre, the frame's
        hard shadow) that arrive; 0.0 where the pixel does not face the light, 1.0 on a miss. vis: a device tensor (or
        a raw address) holding the planes plane_stride floats apart (0: nrows * width, back to back). Each plane feeds
        ao_accumulate / ao_atrous as an AO plane does; host_shadow_rays gives the rays. nlights: the number of planes
        the tensor is checked to hold (None: the count set_shading was given through this Context)."""
        rp, nr, _keep = self._rows_arg(rows, height)
        self._vis_planes("dispatch_shadow", vis, nr * width, plane_stride, nlights)
        p = rt_shadow_params(samples, seed, light_radius, tmin)
        self._check(self._lib.rt_dispatch_shadow(self._h, width, height, rp, nr, ctypes.byref(p), _ptr(vis),
                                                 plane_stride, stream), "rt_dispatch_shadow")

    def shade_resolve(self, width: int, height: int, hits, normal, object, color_out, vis=None, ao=None,  # noqa: A002
                      rgba8_out=None, vis_stride: int = 0, stream: Optional[int] = None,
                      nlights: Optional[int] = None):
        """rt_shade_resolve: the colour frame from dispatch_gbuffer's hits, normal and object planes (whole frames),
        dispatch_shadow's visibility planes (vis, vis_stride floats apart, 0: width * height; None: every light fully
        visible) and an AO plane (ao; None: 1), under the context's camera and lights. color_out: width * height x 4
        floats (alpha 1), the format upscale takes; rgba8_out: optional width * height x 4 bytes. With vis from
        dispatch_shadow(samples=1, light_radius=0) and ao None the frame is dispatch()'s RT_SHADE_LAMBERT_SHADOW frame
        bit for bit; with vis None, its RT_SHADE_PRIMARY frame. nlights: as for dispatch_shadow."""
        n, m = width * height, "shade_resolve"
        self._vis_planes(m, vis, n, vis_stride, nlights)
        inp = rt_resolve_inputs(self._plane(m, "hits", hits, 4 * n), self._plane(m, "normal", normal, 4 * n),
                                self._plane(m, "object", object, 2 * n), _ptr(vis), vis_stride,
                                self._plane(m, "ao", ao, n))
        out8 = rgba8_out.view(torch.int32) if isinstance(rgba8_out, torch.Tensor) and rgba8_out.dtype == torch.uint8 \
            else rgba8_out
        self._check(self._lib.rt_shade_resolve(self._h, width, height, ctypes.byref(inp),
                                               self._plane(m, "color_out", color_out, 4 * n),
                                               self._plane(m, "rgba8_out", out8, n), stream), "rt_shade_resolve")

    def shade_resolve_pbr(self, width: int, height: int, hits, normal, object, color_out, materials,  # noqa: A002
                          instance_material=None, vis=None, ao=None, refl=None, rgba8_out=None, vis_stride: int = 0,
                          stream: Optional[int] = None, nlights: Optional[int] = None):
        """rt_shade_resolve_pbr: shade_resolve with the RT_SHADE_REF hit programs in place of the grey Lambert term and
        a material per instance. materials: a sequence of 6-tuples, set_shading's material format (1..32 of them),
        copied during the call; instance_material: a device tensor of uint32 / int32 material indices by instance
        index (the object plane's first word: the position in tlas_build's list), or None (material 0 everywhere); an
        index out of either range means material 0. refl: dispatch_reflection's radiance plane (width * height x 4
        floats) or None: where given, a model pixel's colour is lerped towards it by its material's reflectivity. The
        plane group is shaded as the reference's PlaneClosestHit (light 0, no material). With one material and no
        optional plane the model and miss pixels are dispatch()'s RT_SHADE_REF frame bit for bit; with vis from
        dispatch_shadow(samples=1, light_radius=0) the plane pixels are too. nlights: as for dispatch_shadow."""
        n, m = width * height, "shade_resolve_pbr"
        self._vis_planes(m, vis, n, vis_stride, nlights)
        inp = rt_resolve_pbr_inputs(self._plane(m, "hits", hits, 4 * n), self._plane(m, "normal", normal, 4 * n),
                                    self._plane(m, "object", object, 2 * n), _ptr(vis), vis_stride,
                                    self._plane(m, "ao", ao, n), self._plane(m, "refl", refl, 4 * n))
        mats, nm = _materials_array(materials)
        ninst = 0
        if instance_material is not None:
            if isinstance(instance_material, int):
                raise ValueError(f"{m}: instance_material must be a tensor (its length is the map's size)")
            if instance_material.element_size() != 4 or not instance_material.is_contiguous():
                raise ValueError(f"{m}: instance_material must be a contiguous tensor of 32-bit elements")
            ninst = instance_material.numel()
        table = rt_material_table(mats, nm, _ptr(instance_material), ninst)
        out8 = rgba8_out.view(torch.int32) if isinstance(rgba8_out, torch.Tensor) and rgba8_out.dtype == torch.uint8 \
            else rgba8_out
        self._check(self._lib.rt_shade_resolve_pbr(self._h, width, height, ctypes.byref(inp), ctypes.byref(table),
                                                   self._plane(m, "color_out", color_out, 4 * n),
                                                   self._plane(m, "rgba8_out", out8, n), stream),
                    "rt_shade_resolve_pbr")

    def dispatch_reflection(self, width: int, height: int, radiance, samples: int = 1, roughness: float = 0.0,
                            tmax: float = 1000.0, shadow_tmin: float = 0.01, seed: int = 0, hits=None,
                            rows: Optional[np.ndarray] = None, stream: Optional[int] = None):
        """rt_dispatch_reflection: the reflections of the frame dispatch_gbuffer describes, 4 floats per pixel (nrows *
        width entries in dispatch()'s compact row order): the mean colour of `samples` (1..64) reflection rays about
        the mirror direction of the G-buffer's normal (roughness in [0, 1]; 0: the mirror ray itself), each shaded as a
        Lambert-shadow sample under set_shading's lights or with the miss colour, and in .w their mean distance; four
        zeros on a primary miss. hits: optional, ray 0's record per pixel as trace_rays writes it (4 words). Device
        tensors (or raw addresses). host_reflection_rays and host_reflection_radiance give the rays and the plane."""
        rp, nr, _keep = self._rows_arg(rows, height)
        g = rt_reflection_planes()
        self._set_planes(g, "dispatch_reflection", nr * width, (("radiance", radiance, 4), ("hits", hits, 4)))
        p = rt_reflection_params(samples, seed, roughness, tmax, shadow_tmin)
        self._check(self._lib.rt_dispatch_reflection(self._h, width, height, rp, nr, ctypes.byref(p), ctypes.byref(g),
                                                     stream), "rt_dispatch_reflection")

    def dispatch_reflection_pbr(self, width: int, height: int, radiance, materials, instance_material=None,
                                samples: int = 1, roughness: float = 0.0, tmax: float = 1000.0,
                                shadow_tmin: float = 0.01, seed: int = 0, flags: int = 0, hits=None,
                                rows: Optional[np.ndarray] = None, stream: Optional[int] = None):
        """rt_dispatch_reflection_pbr: dispatch_reflection with the RT_SHADE_REF hit programs at each reflected hit: the
        plane group as the reference's PlaneClosestHit (light 0, one shadow ray), every other group as ClosestHit's
        surface colour with the hit instance's material. materials, instance_material: as for shade_resolve_pbr.
        flags: RT_REFLECT_FRAME_RAY (the frame kernels' mirror direction, about the normal as stored: what makes
        shade_resolve_pbr(refl=...) equal dispatch()'s reflective RT_SHADE_REF frame bit for bit where the mirror chain
        is one bounce long) and RT_REFLECT_SHADOW_MODELS (a shadow ray per light a reflected model hit faces). With
        flags 0 the rays, the hits plane and radiance's .w are dispatch_reflection's. host_reflection_rays_flags and
        host_reflection_radiance_pbr give the rays and the plane."""
        m = "dispatch_reflection_pbr"
        rp, nr, _keep = self._rows_arg(rows, height)
        g = rt_reflection_planes()
        self._set_planes(g, m, nr * width, (("radiance", radiance, 4), ("hits", hits, 4)))
        mats, nm = _materials_array(materials)
        ninst = 0
        if instance_material is not None:
            if isinstance(instance_material, int):
                raise ValueError(f"{m}: instance_material must be a tensor (its length is the map's size)")
            if instance_material.element_size() != 4 or not instance_material.is_contiguous():
                raise ValueError(f"{m}: instance_material must be a contiguous tensor of 32-bit elements")
            ninst = instance_material.numel()
        table = rt_material_table(mats, nm, _ptr(instance_material), ninst)
        p = rt_reflection_pbr_params(samples, seed, roughness, tmax, shadow_tmin, flags)
        self._check(self._lib.rt_dispatch_reflection_pbr(self._h, width, height, rp, nr, ctypes.byref(p),
                                                         ctypes.byref(table), ctypes.byref(g), stream),
                    "rt_dispatch_reflection_pbr")

    def _material_table(self, m: str, materials, instance_material):
        """The rt_material_table of a call from set_shading-format materials and a device map (or None); the returned
        array must outlive the call."""
        mats, nm = _materials_array(materials)
        ninst = 0
        if instance_material is not None:
            if isinstance(instance_material, int):
                raise ValueError(f"{m}: instance_material must be a tensor (its length is the map's size)")
            if instance_material.element_size() != 4 or not instance_material.is_contiguous():
                raise ValueError(f"{m}: instance_material must be a contiguous tensor of 32-bit elements")
            ninst = instance_material.numel()
        return rt_material_table(mats, nm, _ptr(instance_material), ninst), mats

    def dispatch_reflection_chain(self, width: int, height: int, radiance, materials, instance_material=None,
                                  samples: int = 1, roughness: float = 0.0, tmax: float = 1000.0,
                                  shadow_tmin: float = 0.01, seed: int = 0, flags: int = 0, max_bounces: int = 4,
                                  hits=None, rows: Optional[np.ndarray] = None, stream: Optional[int] = None):
        """rt_dispatch_reflection_chain: dispatch_reflection_pbr whose reflected model hits reflect in turn, up to
        max_bounces (1..RT_MAX_REFLECTION_BOUNCES) rays per sample: a hit whose material's reflectivity is not 0 sends
        the frame kernels' mirror ray and its colour is lerped towards what that ray returns, innermost first. Every
        other argument is dispatch_reflection_pbr's. With max_bounces 1 the planes are that pass's bytes; with 18 and
        RT_REFLECT_FRAME_RAY, shade_resolve_pbr(refl=...) equals dispatch()'s reflective RT_SHADE_REF frame at every
        pixel. radiance's .w and hits describe the first rays. At max_bounces 1 a launch measures level with
        dispatch_reflection_pbr; each further bounce costs its rays. host_reflection_chain_rays and
        host_reflection_chain_radiance give the rays and the plane."""
        m = "dispatch_reflection_chain"
        rp, nr, _keep = self._rows_arg(rows, height)
        g = rt_reflection_planes()
        self._set_planes(g, m, nr * width, (("radiance", radiance, 4), ("hits", hits, 4)))
        table, _mats = self._material_table(m, materials, instance_material)
        p = rt_reflection_chain_params(samples, seed, roughness, tmax, shadow_tmin, flags, max_bounces)
        self._check(self._lib.rt_dispatch_reflection_chain(self._h, width, height, rp, nr, ctypes.byref(p),
                                                           ctypes.byref(table), ctypes.byref(g), stream),
                    "rt_dispatch_reflection_chain")

    def dispatch_indirect(self, width: int, height: int, radiance, materials, instance_material=None,
                          samples: int = 1, tmax: float = 1000.0, shadow_tmin: float = 0.01, seed: int = 0,
                          flags: int = RT_REFLECT_SHADOW_MODELS, hits=None, rows: Optional[np.ndarray] = None,
                          stream: Optional[int] = None):
        """rt_dispatch_indirect: one bounce of diffuse indirect light for the frame dispatch_gbuffer describes, 4 floats
        per pixel (nrows * width entries in dispatch()'s compact row order): the mean colour of `samples` (1..64)
        cosine-weighted rays about the facing normal, each shaded as dispatch_reflection_pbr shades a reflection ray
        (the hit instance's material; the miss colour where it hits nothing), and in .w their mean distance; four zeros
        on a primary miss. materials, instance_material, hits: as for dispatch_reflection_pbr. flags:
        RT_REFLECT_SHADOW_MODELS (the default: an unshadowed bounce leaks light) or 0. The plane feeds
        radiance_accumulate / radiance_atrous and then shade_resolve_gi(indirect=...). host_indirect_rays gives the rays,
        host_reflection_radiance_pbr (roughness 0) the plane."""
        m = "dispatch_indirect"
        rp, nr, _keep = self._rows_arg(rows, height)
        g = rt_reflection_planes()
        self._set_planes(g, m, nr * width, (("radiance", radiance, 4), ("hits", hits, 4)))
        table, _mats = self._material_table(m, materials, instance_material)
        p = rt_indirect_params(samples, seed, tmax, shadow_tmin, flags)
        self._check(self._lib.rt_dispatch_indirect(self._h, width, height, rp, nr, ctypes.byref(p),
                                                   ctypes.byref(table), ctypes.byref(g), stream),
                    "rt_dispatch_indirect")

    def shade_resolve_gi(self, width: int, height: int, hits, normal, object, color_out, materials,  # noqa: A002
                         instance_material=None, vis=None, ao=None, refl=None, rgba8_out=None, vis_stride: int = 0,
                         stream: Optional[int] = None, nlights: Optional[int] = None, indirect=None,
                         indirect_scale: float = 1.0):
        """rt_shade_resolve_gi: shade_resolve_pbr with a diffuse indirect term. indirect: dispatch_indirect's radiance
        plane (width * height x 4 floats, filtered or not) or None; where given, a model pixel gains
        ((1 - metallic) * albedo) * indirect * indirect_scale per channel before the lerp towards refl, a plane pixel
        indirect * indirect_scale, a miss nothing. indirect_scale: finite, >= 0. With indirect None, a plane of zeros
        or scale 0 the frame is shade_resolve_pbr's bit for bit."""
        n, m = width * height, "shade_resolve_gi"
        self._vis_planes(m, vis, n, vis_stride, nlights)
        inp = rt_resolve_gi_inputs(self._plane(m, "hits", hits, 4 * n), self._plane(m, "normal", normal, 4 * n),
                                   self._plane(m, "object", object, 2 * n), _ptr(vis), vis_stride,
                                   self._plane(m, "ao", ao, n), self._plane(m, "refl", refl, 4 * n),
                                   self._plane(m, "indirect", indirect, 4 * n), indirect_scale)
        table, _mats = self._material_table(m, materials, instance_material)
        out8 = rgba8_out.view(torch.int32) if isinstance(rgba8_out, torch.Tensor) and rgba8_out.dtype == torch.uint8 \
            else rgba8_out
        self._check(self._lib.rt_shade_resolve_gi(self._h, width, height, ctypes.byref(inp), ctypes.byref(table),
                                                  self._plane(m, "color_out", color_out, 4 * n),
                                                  self._plane(m, "rgba8_out", out8, n), stream),
                    "rt_shade_resolve_gi")

    def reflection_composite(self, width: int, height: int, color_in, radiance, hits, normal, color_out,
                             strength: float = 1.0, f0: float = 0.04, rgba8_out=None, stream: Optional[int] = None):
        """rt_reflection_composite: color_out = lerp(color_in, radiance, strength * F) per pixel, F Schlick's Fresnel
        term (f0 at normal incidence) at the G-buffer's normal under the context's camera; color_in where the primary
        ray missed. Whole frames: color_in, radiance, normal, color_out width * height x 4 floats, hits the primary
        dispatch_gbuffer hits plane; color_out may be color_in; rgba8_out: optional width * height x 4 bytes. strength
        0 returns color_in bit for bit; f0 1 weights every pixel by strength exactly."""
        n, m = width * height, "reflection_composite"
        out8 = rgba8_out.view(torch.int32) if isinstance(rgba8_out, torch.Tensor) and rgba8_out.dtype == torch.uint8 \
            else rgba8_out
        p = rt_reflection_composite_params(strength, f0)
        self._check(self._lib.rt_reflection_composite(
            self._h, width, height, ctypes.byref(p), self._plane(m, "color_in", color_in, 4 * n),
            self._plane(m, "radiance", radiance, 4 * n), self._plane(m, "hits", hits, 4 * n),
            self._plane(m, "normal", normal, 4 * n), self._plane(m, "color_out", color_out, 4 * n),
            self._plane(m, "rgba8_out", out8, n), stream), "rt_reflection_composite")

    @staticmethod
    def _plane(method: str, name: str, t, words: int):
        """A filter plane's address: a contiguous tensor of exactly `words` 32-bit elements, a raw address, or None."""
        if t is not None and not isinstance(t, int):
            if t.element_size() != 4 or t.numel() != words or not t.is_contiguous():
                raise ValueError(f"{method}: {name} must be a contiguous tensor of {words} 32-bit elements, got "
                                 f"{t.numel()} of {t.element_size()} bytes")
        return _ptr(t)

    def denoise_guide(self, n: int, normal, depth, guide, depth_stride: int = 4, stream: Optional[int] = None):
        """rt_denoise_guide: the AO filter's guide plane, (unit normal, depth) or four zeros per pixel. normal: n x 4
        floats (dispatch_gbuffer's normal plane); depth: a raw address, or a tensor whose element 0 is the first
        depth (motion.view(-1)[3:] for w_cur, hits.view(torch.float32) for t), read every depth_stride floats; guide: n
        x 4 floats. Both frames' guides must come from w_cur when they feed ao_accumulate."""
        d = depth if depth is None or isinstance(depth, int) else depth.data_ptr()
        self._check(self._lib.rt_denoise_guide(self._h, n, self._plane("denoise_guide", "normal", normal, 4 * n), d,
                                               depth_stride, self._plane("denoise_guide", "guide", guide, 4 * n),
                                               stream), "rt_denoise_guide")

    def ao_accumulate(self, width: int, height: int, ao_cur, motion, guide_cur, ao_out, hist_out, ao_prev=None,
                      hist_prev=None, guide_prev=None, max_history: int = 32, depth_tol: float = 0.02,
                      normal_cos: float = 0.9, stream: Optional[int] = None):
        """rt_ao_accumulate: the current AO plane blended into the previous frame's, fetched through the motion plane
        and tested against the previous guide; hist_out counts the frames a pixel has accumulated (0: no surface).
        ao_prev, hist_prev, guide_prev all None: the first frame. ao_out may be ao_cur."""
        n, m = width * height, "ao_accumulate"
        p = rt_ao_temporal_params(max_history, depth_tol, normal_cos)
        self._check(self._lib.rt_ao_accumulate(
            self._h, width, height, ctypes.byref(p), self._plane(m, "ao_cur", ao_cur, n),
            self._plane(m, "motion", motion, 4 * n), self._plane(m, "guide_cur", guide_cur, 4 * n),
            self._plane(m, "ao_prev", ao_prev, n), self._plane(m, "hist_prev", hist_prev, n),
            self._plane(m, "guide_prev", guide_prev, 4 * n), self._plane(m, "ao_out", ao_out, n),
            self._plane(m, "hist_out", hist_out, n), stream), "rt_ao_accumulate")

    def ao_atrous(self, width: int, height: int, ao_in, guide, ao_out, tmp=None, iterations: int = 3,
                  depth_tol: float = 0.02, normal_cos: float = 0.9, stream: Optional[int] = None):
        """rt_ao_atrous: `iterations` (1..5) passes of the edge-aware 5 x 5 a-trous filter, steps 1, 2, 4, ...; the
        result lands in ao_out, ao_in is not written; tmp (width * height floats) is needed from two iterations on."""
        n, m = width * height, "ao_atrous"
        p = rt_ao_atrous_params(iterations, depth_tol, normal_cos)
        self._check(self._lib.rt_ao_atrous(self._h, width, height, ctypes.byref(p), self._plane(m, "ao_in", ao_in, n),
                                           self._plane(m, "guide", guide, 4 * n), self._plane(m, "ao_out", ao_out, n),
                                           self._plane(m, "tmp", tmp, n), stream), "rt_ao_atrous")

    @classmethod
    def _plane_set(cls, method: str, name: str, planes, words: int):
        """A set of filter planes -> (the host table of their addresses, their count). planes: a 2-D tensor whose rows
        are the planes, or a sequence of 1-D tensors (raw addresses and None are passed through, for the library to
        judge); every row is checked as _plane checks a plane. None -> (None, 0)."""
        if planes is None:
            return None, 0
        if not isinstance(planes, (list, tuple)):
            if planes.dim() != 2:
                raise ValueError(f"{method}: {name} must be a 2-D tensor of planes or a sequence of planes")
            planes = [planes[r] for r in range(planes.shape[0])]
        ptrs = [cls._plane(method, f"{name}[{r}]", t, words) for r, t in enumerate(planes)]
        return (ctypes.c_void_p * len(ptrs))(*ptrs), len(ptrs)

    def ao_accumulate_planes(self, width: int, height: int, cur, motion, guide_cur, out, hist_out, prev=None,
                             hist_prev=None, guide_prev=None, max_history: int = 32, depth_tol: float = 0.02,
                             normal_cos: float = 0.9, stream: Optional[int] = None):
        """rt_ao_accumulate_planes: ao_accumulate for up to 17 planes in one launch (a frame's visibility planes and
        its AO plane), which share the motion plane, the guides and ONE history plane; every out plane equals
        ao_accumulate's bit for bit. cur, out, prev: plane sets (a 2-D tensor whose rows are the planes, or a sequence
        of 1-D tensors, which need not be neighbours in memory). prev, hist_prev, guide_prev all None: the first
        frame. out[p] may be cur[p]; no other two planes of the call may be the same."""
        n, m = width * height, "ao_accumulate_planes"
        tc, count = self._plane_set(m, "cur", cur, n)
        to, no = self._plane_set(m, "out", out, n)
        tp, np_ = self._plane_set(m, "prev", prev, n)
        if no != count or (prev is not None and np_ != count):
            raise ValueError(f"{m}: cur has {count} planes, out {no}" + ("" if prev is None else f", prev {np_}"))
        p = rt_ao_temporal_params(max_history, depth_tol, normal_cos)
        self._check(self._lib.rt_ao_accumulate_planes(
            self._h, width, height, ctypes.byref(p), count, tc, self._plane(m, "motion", motion, 4 * n),
            self._plane(m, "guide_cur", guide_cur, 4 * n), tp, self._plane(m, "hist_prev", hist_prev, n),
            self._plane(m, "guide_prev", guide_prev, 4 * n), to, self._plane(m, "hist_out", hist_out, n), stream),
            "rt_ao_accumulate_planes")

    def ao_atrous_planes(self, width: int, height: int, planes_in, guide, planes_out, tmp=None, iterations: int = 3,
                         depth_tol: float = 0.02, normal_cos: float = 0.9, stream: Optional[int] = None):
        """rt_ao_atrous_planes: ao_atrous for up to 17 planes under one guide, one launch per iteration; every
        planes_out plane equals ao_atrous's bit for bit, planes_in is not written. planes_in, planes_out, tmp: plane
        sets as ao_accumulate_planes'; tmp (one plane per input plane) is needed from two iterations on."""
        n, m = width * height, "ao_atrous_planes"
        ti, count = self._plane_set(m, "planes_in", planes_in, n)
        to, no = self._plane_set(m, "planes_out", planes_out, n)
        tt, nt = self._plane_set(m, "tmp", tmp, n)
        if no != count or (tmp is not None and nt != count):
            raise ValueError(f"{m}: planes_in has {count} planes, planes_out {no}" +
                             ("" if tmp is None else f", tmp {nt}"))
        p = rt_ao_atrous_params(iterations, depth_tol, normal_cos)
        self._check(self._lib.rt_ao_atrous_planes(self._h, width, height, ctypes.byref(p), count, ti,
                                                  self._plane(m, "guide", guide, 4 * n), to, tt, stream),
                    "rt_ao_atrous_planes")

    def radiance_accumulate(self, width: int, height: int, rad_cur, motion, guide_cur, rad_out, moments_out,
                            rad_prev=None, moments_prev=None, guide_prev=None, max_history: int = 32,
                            depth_tol: float = 0.02, normal_cos: float = 0.9, stream: Optional[int] = None):
        """rt_radiance_accumulate: ao_accumulate for a plane of 4-float entries (dispatch_reflection's radiance), all
        four channels blended alike, with the luminance moments (m1, m2, hist, var) in moments_out: the variance
        radiance_atrous reads. Every plane is width * height x 4 floats. rad_prev, moments_prev, guide_prev all None:
        the first frame. No output may be an input (rad_cur's neighbours are read)."""
        n, m = 4 * width * height, "radiance_accumulate"
        p = rt_radiance_temporal_params(max_history, depth_tol, normal_cos)
        self._check(self._lib.rt_radiance_accumulate(
            self._h, width, height, ctypes.byref(p), self._plane(m, "rad_cur", rad_cur, n),
            self._plane(m, "motion", motion, n), self._plane(m, "guide_cur", guide_cur, n),
            self._plane(m, "rad_prev", rad_prev, n), self._plane(m, "moments_prev", moments_prev, n),
            self._plane(m, "guide_prev", guide_prev, n), self._plane(m, "rad_out", rad_out, n),
            self._plane(m, "moments_out", moments_out, n), stream), "rt_radiance_accumulate")

    def radiance_atrous(self, width: int, height: int, rad_in, moments, guide, rad_out, var_out, tmp=None,
                        var_tmp=None, iterations: int = 3, depth_tol: float = 0.02, normal_cos: float = 0.9,
                        sigma_l: float = 4.0, stream: Optional[int] = None):
        """rt_radiance_atrous: `iterations` (1..5) passes of the a-trous filter over a plane of 4-float entries, the
        luminance weight scaled by the variance (moments' .w, filtered along with the colour); the result lands in
        rad_out / var_out, rad_in and moments are not written; tmp (width * height x 4 floats) and var_tmp (width *
        height floats) are needed from two iterations on."""
        n, m = width * height, "radiance_atrous"
        p = rt_radiance_atrous_params(iterations, depth_tol, normal_cos, sigma_l)
        self._check(self._lib.rt_radiance_atrous(
            self._h, width, height, ctypes.byref(p), self._plane(m, "rad_in", rad_in, 4 * n),
            self._plane(m, "moments", moments, 4 * n), self._plane(m, "guide", guide, 4 * n),
            self._plane(m, "rad_out", rad_out, 4 * n), self._plane(m, "var_out", var_out, n),
            self._plane(m, "tmp", tmp, 4 * n), self._plane(m, "var_tmp", var_tmp, n), stream), "rt_radiance_atrous")

    def reflection_motion(self, width: int, height: int, hits, guide_cur, motion, dist, camera, prev_camera,
                          motion_out, guide_prev=None, class_out=None, dist_stride: int = 4, share: float = 1.0,
                          static_tol: float = REFLECTION_MOTION_STATIC_TOL, depth_tol: float = 0.02,
                          normal_cos: float = 0.9, stream: Optional[int] = None):
        """rt_reflection_motion: the motion plane of what is seen IN a reflector (the virtual reflected point's), to
        pass to radiance_accumulate in place of the G-buffer's surface motion when the plane is a reflection. hits:
        dispatch_gbuffer's hits plane; guide_cur, motion, motion_out: width * height x 4 floats; dist: a raw address, or
        a tensor whose element 0 is the first distance (rad.view(-1)[3:] for a reflection plane's .w), read every
        dist_stride floats; camera / prev_camera: the two frames' 64-float camera buffers (host arrays); guide_prev: the
        previous frame's guide or None; class_out: width * height bytes (uint8) or None. A pixel whose reflector moved,
        whose virtual point cannot be seen from the previous camera or at which no history would be found keeps its
        surface motion bit for bit. static_tol's default, 2^-4 px, is 16 x the largest distance measured between
        the static point's entry and the motion plane's on static geometry (0.00256 px, C2F at 1080p), rounded up to a
        power of two."""
        n, m = width * height, "reflection_motion"
        d = dist if dist is None or isinstance(dist, int) else dist.data_ptr()
        if class_out is not None and not isinstance(class_out, int):
            if class_out.element_size() != 1 or class_out.numel() != n or not class_out.is_contiguous():
                raise ValueError(f"{m}: class_out must be a contiguous tensor of {n} bytes")
        cb = None if camera is None else _f32(camera, 64)
        pcb = None if prev_camera is None else _f32(prev_camera, 64)
        p = rt_reflection_motion_params(share, static_tol, depth_tol, normal_cos)
        self._check(self._lib.rt_reflection_motion(
            self._h, width, height, ctypes.byref(p), self._plane(m, "hits", hits, 4 * n),
            self._plane(m, "guide_cur", guide_cur, 4 * n), self._plane(m, "motion", motion, 4 * n), d, dist_stride,
            self._plane(m, "guide_prev", guide_prev, 4 * n), _vp(cb), _vp(pcb), self._plane(m, "motion_out", motion_out, 4 * n), _ptr(class_out),
            stream), "rt_reflection_motion")

    def radiance_accumulate_reflection(self, width: int, height: int, rad_cur, motion, guide_cur, hits, camera,
                                       prev_camera, rad_out, moments_out, rad_prev=None, moments_prev=None,
                                       guide_prev=None, max_history: int = 32, depth_tol: float = 0.02,
                                       normal_cos: float = 0.9, share: float = 1.0,
                                       static_tol: float = REFLECTION_MOTION_STATIC_TOL,
                                       stream: Optional[int] = None):
        """rt_radiance_accumulate_reflection: reflection_motion (with dist = rad_cur's .w and this call's guide_prev,
        depth_tol and normal_cos) and radiance_accumulate in one launch, bit-equal to the two; the motion entry stays
        in registers. Without the previous planes it is radiance_accumulate itself."""
        n, m = 4 * width * height, "radiance_accumulate_reflection"
        cb = None if camera is None else _f32(camera, 64)
        pcb = None if prev_camera is None else _f32(prev_camera, 64)
        p = rt_radiance_temporal_params(max_history, depth_tol, normal_cos)
        q = rt_reflection_motion_params(share, static_tol, depth_tol, normal_cos)
        self._check(self._lib.rt_radiance_accumulate_reflection(
            self._h, width, height, ctypes.byref(p), ctypes.byref(q), self._plane(m, "rad_cur", rad_cur, n),
            self._plane(m, "motion", motion, n), self._plane(m, "guide_cur", guide_cur, n),
            self._plane(m, "hits", hits, n), _vp(cb), _vp(pcb), self._plane(m, "rad_prev", rad_prev, n),
            self._plane(m, "moments_prev", moments_prev, n), self._plane(m, "guide_prev", guide_prev, n),
            self._plane(m, "rad_out", rad_out, n), self._plane(m, "moments_out", moments_out, n), stream),
            "rt_radiance_accumulate_reflection")

    def upscale(self, render_width: int, render_height: int, width: int, height: int, color_cur, motion_cur, color_out,
                hist_out, motion_prev=None, color_prev=None, hist_prev=None, rgba8_out=None, jitter_cur=(0.0, 0.0),
                jitter_prev=(0.0, 0.0), max_history: int = 16, depth_tol: float = 0.02,
                stream: Optional[int] = None):
        """rt_upscale: a width x height frame reconstructed from the jittered render_width x render_height colour frame
        (dispatch's rgba32f under camera_jitter's camera), its motion plane and the previous call's color_out /
        hist_out, fetched through the motion. motion_prev, color_prev, hist_prev all None: the first frame. rgba8_out:
        optional width * height x 4 bytes."""
        n, N, m = render_width * render_height, width * height, "upscale"
        p = _upscale_params(jitter_cur, jitter_prev, max_history, depth_tol)
        self._check(self._lib.rt_upscale(
            self._h, render_width, render_height, width, height, ctypes.byref(p),
            self._plane(m, "color_cur", color_cur, 4 * n), self._plane(m, "motion_cur", motion_cur, 4 * n),
            self._plane(m, "motion_prev", motion_prev, 4 * n), self._plane(m, "color_prev", color_prev, 4 * N),
            self._plane(m, "hist_prev", hist_prev, N), self._plane(m, "color_out", color_out, 4 * N),
            self._plane(m, "hist_out", hist_out, N),
            self._plane(m, "rgba8_out", rgba8_out.view(torch.int32) if isinstance(rgba8_out, torch.Tensor)
                        and rgba8_out.dtype == torch.uint8 else rgba8_out, N), stream), "rt_upscale")

    def pick(self, width: int, height: int, x: int, y: int) -> Optional[dict]:
        """What the camera ray through the centre of pixel (x, y) of a width x height frame hits: None on a miss, else
        t, instance_id, instance (index in the tlas_build list), hit_group, primitive, uv and the world normal (see
        rt_gbuffer). One one-row G-buffer launch on torch's current stream, synchronised. (torch's default stream has
        the handle 0, which the library reads as "the context's stream", a non-blocking one: so the wait is for the
        device, not for torch's stream, which the launch may not be on.)"""
        if not (0 <= x < width and 0 <= y < height):
            raise ValueError(f"pick: pixel ({x}, {y}) outside {width} x {height}")
        dev = f"cuda:{self.device}"
        hits = torch.empty((width, 4), dtype=torch.int32, device=dev)
        uv = torch.empty((width, 2), dtype=torch.float32, device=dev)
        nrm = torch.empty((width, 4), dtype=torch.float32, device=dev)
        obj = torch.empty((width, 2), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(self.device)
        self.dispatch_gbuffer(width, height, hits, uv, nrm, obj, rows=np.array([y], np.uint32),
                              stream=stream.cuda_stream)
        torch.cuda.synchronize(self.device)
        h = hits[x].cpu().numpy().view(np.uint32)
        if h[3] == 0:
            return None
        o = obj[x].cpu().numpy().view(np.uint32)
        return {"t": float(h[0:1].view(np.float32)[0]), "instance_id": int(h[1]), "instance": int(o[0]),
                "hit_group": int(o[1]), "primitive": int(h[2]), "uv": tuple(float(v) for v in uv[x].cpu().numpy()),
                "normal": tuple(float(v) for v in nrm[x, :3].cpu().numpy())}

    def trace_rays(self, rays, n: int, any_hit: bool, hits, uv=None, stream: Optional[int] = None,
                   cull_back: bool = False, cull_front: bool = False):
        flags = (RT_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH if any_hit else 0) | \
            (RT_RAY_FLAG_CULL_BACK_FACING_TRIANGLES if cull_back else 0) | \
            (RT_RAY_FLAG_CULL_FRONT_FACING_TRIANGLES if cull_front else 0)
        self._check(self._lib.rt_trace_rays(self._h, _ptr(rays), n, flags, _ptr(hits), _ptr(uv), stream),
                    "rt_trace_rays")

    def raster_draw(self, draws: Sequence[int], width: int, height: int, rgba8, depth=None, object_to_world=None,
                    stream: Optional[int] = None):
        """Raster fallback (rt_raster_draw; shaders/shaders.hlsl:41-59, D3D12HelloTriangle.cpp:513-540):
        draws the BLAS vertex buffers in order with the current camera into rgba8 (H x W x 4 device
        tensor) and optionally depth (H x W float32 device tensor)."""
        d = np.ascontiguousarray(draws, dtype=np.uint32)
        x = None if object_to_world is None else _f32(object_to_world, 12)
        self._check(self._lib.rt_raster_draw(self._h, d.ctypes.data_as(_UP), len(d),
                                             None if x is None else _fptr(x), width, height, _ptr(rgba8),
                                             _ptr(depth), stream), "rt_raster_draw")

    def forget_stream(self, stream: int):
        """rt_forget_stream: call before destroying a stream this context launched on (see rt_api.h)."""
        self._check(self._lib.rt_forget_stream(self._h, stream), "rt_forget_stream")

    def assemble_strips(self, width: int, height: int, nranks: int, strip_rows_: int, gathered, out,
                        stream: Optional[int] = None):
        self._check(self._lib.rt_assemble_strips(self._h, width, height, nranks, strip_rows_, _ptr(gathered), _ptr(out),
                                           stream), "rt_assemble_strips")
