"""ptamd — Python binding of the C-ABI in include/pt_api.h (libptamd.so).

This is plumbing only: ctypes declarations, numpy views of the C structs and thin
wrappers.  The renderer itself is the HIP library; nothing here computes radiance, and
there is no CPU fallback — if libptamd.so is missing or a HIP call fails, these functions
raise.  torch is used (by ptamd.dist and bench.py) for device buffers, streams and
torch.distributed only.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("PTAMD_LIB") or os.path.join(PKG_ROOT, "libptamd.so")      # PTAMD_LIB: A/B builds of the same library

TRACE_STAT_LAUNCHES = 2700      # csrc/pt_device.h: kStatLaunches, the wf_trace launches the diagnostic counter buffer has a slot for (later ones share the last)
PRIM_FLOATS = 84      # sizeof(PtPrimitive) / 4   (3 x 112-byte Vertex, include/mesh.h:21-37)
TRI_FLOATS = 88       # sizeof(PtTriangle) / 4
NODE_BYTES = 40       # sizeof(PtBVHNode)        (CudaBVHNode, include/CudaPrimitive.cuh:237-247)
SPHERE_FLOATS = 16
TILE = 8

NODE_DTYPE = np.dtype([("bMin", "<f4", 3), ("bMax", "<f4", 3), ("childL", "<i4"), ("childR", "<i4"),
                       ("primStart", "<i4"), ("primEnd", "<i4")])
assert NODE_DTYPE.itemsize == NODE_BYTES


class PtError(RuntimeError):
    pass


class PtCamera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("forward", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3),
                ("fovy_deg", C.c_float), ("aspect", C.c_float), ("W", C.c_int32), ("H", C.c_int32)]


class PtParams(C.Structure):
    _fields_ = [("passes", C.c_int32), ("spp_per_pass", C.c_int32), ("max_bounce", C.c_int32), ("rr_bounce", C.c_int32),
                ("rr_floor", C.c_float), ("max_refract", C.c_int32), ("first_pass", C.c_int32),
                ("rank", C.c_int32), ("world", C.c_int32)]


class PtDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int32)]


class PtErrorEstimate(C.Structure):
    _fields_ = [("rel_rms", C.c_double), ("mean_rel_se", C.c_double), ("pixels", C.c_int64), ("skipped", C.c_int64)]


class PtTileError(C.Structure):
    _fields_ = [("mean_rel_se", C.c_double), ("pixels", C.c_int32), ("skipped", C.c_int32)]


class PtAdaptiveReport(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("tiles", C.c_int32), ("tiles_converged", C.c_int32), ("tile_passes", C.c_int64),
                ("max_tile_err", C.c_double)]


TILE_ERROR_DTYPE = np.dtype([("mean_rel_se", "<f8"), ("pixels", "<i4"), ("skipped", "<i4")])      # PtTileError as a numpy record


class PtTreeInfo(C.Structure):
    _fields_ = [("n_wide", C.c_int32), ("n_quad", C.c_int32), ("depth", C.c_int32), ("quad_depth", C.c_int32), ("rebuilds", C.c_int32)]


class PtRebuildParams(C.Structure):
    _fields_ = [("depth_budget", C.c_int32), ("large_fraction", C.c_float)]


class PtRebuildReport(C.Structure):
    _fields_ = [("n_large", C.c_int32), ("n_flattened_tris", C.c_int32)]


class PtRebuildOptReport(C.Structure):
    _fields_ = [("n_large", C.c_int32), ("n_flattened_tris", C.c_int32), ("n_roots", C.c_int32), ("n_restructured", C.c_int32)]


class PtRayHit(C.Structure):
    _fields_ = [("t", C.c_float), ("prim", C.c_int32)]


HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<i4")])      # PtRayHit as a numpy record
QUERY_CLOSEST, QUERY_ANY = 0, 1


class PtNearest(C.Structure):
    _fields_ = [("dist2", C.c_float), ("prim", C.c_int32)]


NEAREST_DTYPE = np.dtype([("dist2", "<f4"), ("prim", "<i4")])      # PtNearest as a numpy record
NEAREST_CLOSEST, NEAREST_ANY = 0, 1
NEAREST_KMAX = 32      # PT_NEAREST_KMAX: the most slots per point of pt_nearest_k
RAY_HITS_KMAX = 32     # PT_RAY_HITS_KMAX: the most slots per ray of pt_trace_rays_k
HITS_FRONT, HITS_BOTH_SIDES = 0, 1
FILTER_TMIN = 1       # PT_FILTER_TMIN: a ray's 7th float is its near bound


class PtBoxMember(C.Structure):
    _fields_ = [("cls", C.c_float), ("prim", C.c_int32)]


BOX_DTYPE = np.dtype([("cls", "<f4"), ("prim", "<i4")])      # PtBoxMember as a numpy record: cls 0 = inside, 1 = touching
BOX_TOUCHING, BOX_INSIDE = 0, 1
CONVEX_TOUCHING, CONVEX_INSIDE = 0, 1      # PT_CONVEX_TOUCHING, PT_CONVEX_INSIDE
CONVEX_MAX_PLANES = 8                      # PT_CONVEX_MAX_PLANES
SWEEP_CLOSEST, SWEEP_ANY = 0, 1            # PT_SWEEP_CLOSEST, PT_SWEEP_ANY


class PtQueryFilter(C.Structure):
    _fields_ = [("d_prim_bits", C.c_void_p), ("d_query_bits", C.c_void_p), ("d_skip_prim", C.c_void_p), ("bits", C.c_uint32), ("flags", C.c_uint32)]


AOV_FLOATS = 8        # floats per pixel of pt_render_aov: albedo.rgb | normal.xyz | depth | coverage

_lib = None

# every symbol include/pt_api.h declares: (name, restype, argtypes)
_P = C.c_void_p
API = [
    ("pt_params_default", None, [C.POINTER(PtParams)]),
    ("pt_last_error", C.c_char_p, []),
    ("pt_version", C.c_char_p, []),
    ("pt_bvh_build_sah", C.c_int, [_P, C.c_int32, C.POINTER(_P)]),
    ("pt_bvh_free", None, [_P]),
    ("pt_bvh_num_nodes", C.c_int32, [_P]),
    ("pt_bvh_num_tris", C.c_int32, [_P]),
    ("pt_bvh_max_depth", C.c_int32, [_P]),
    ("pt_bvh_nodes", _P, [_P]),
    ("pt_bvh_tris", _P, [_P]),
    ("pt_scene_create", C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pt_scene_destroy", None, [_P]),
    ("pt_scene_num_lights", C.c_int32, [_P]),
    ("pt_scene_device_bytes", C.c_int64, [_P]),
    ("pt_tiles_floats", C.c_int64, [C.POINTER(PtCamera), C.POINTER(PtParams)]),
    ("pt_work_bytes", C.c_int64, [C.POINTER(PtCamera), C.POINTER(PtParams)]),
    ("pt_render_tiles", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), _P, _P, _P]),
    ("pt_untile", C.c_int, [_P, C.POINTER(PtCamera), C.c_int32, _P, _P]),
    ("pt_render", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), _P]),
    ("pt_last_render_ms", C.c_int, [_P, C.POINTER(C.c_float)]),
    ("pt_render_timings", C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    ("pt_comm_unique_id", C.c_int, [_P]),
    ("pt_comm_create", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pt_comm_create_from_file", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pt_comm_create_from_file_tagged", C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pt_comm_destroy", None, [_P]),
    ("pt_comm_rank", C.c_int32, [_P]),
    ("pt_comm_world", C.c_int32, [_P]),
    ("pt_gather_tiles", C.c_int, [_P, _P, C.c_int64, _P, _P]),
    ("pt_gather_frame", C.c_int, [_P, _P, C.POINTER(PtCamera), C.POINTER(PtParams), _P, _P, _P]),
    ("pt_render_split", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), _P, _P]),
    ("pt_tonemap_u8", C.c_int, [_P, C.c_int64, C.c_int32, _P]),
    ("pt_convert_u8", C.c_int, [_P, C.c_int64, _P]),
    ("pt_write_png", C.c_int, [C.c_char_p, _P, C.c_int32, C.c_int32, C.c_int32]),
    ("pt_camera_basis", None, [C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3)]),
    ("pt_scene_gen", C.c_int32, [C.c_int32, C.c_int32, _P, C.c_int32]),
    ("pt_load_obj", C.c_int32, [C.c_char_p, C.c_float, C.POINTER(C.c_float * 3), _P, C.c_int32]),
    ("pt_dbg_raycast", C.c_int, [_P, _P, C.c_int32, _P, _P]),
    ("pt_dbg_bxdf", C.c_int, [C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    ("pt_dbg_rng", C.c_int, [C.c_int32, C.c_uint64, C.c_int32, _P, _P]),
    ("pt_dbg_math", C.c_int, [C.c_int32, _P, C.c_int32, _P]),
    ("pt_dbg_sincos", C.c_int, [C.c_int32, _P, C.c_int32, _P]),
    ("pt_dbg_ray_setup", C.c_int, [C.c_int32, _P, C.c_int32, _P]),
    ("pt_dbg_pixel_dir", C.c_int, [C.c_int32, C.POINTER(PtCamera), _P, C.c_int32, _P]),
    ("pt_dbg_nee", C.c_int, [_P, _P, C.c_int32, _P]),
    ("pt_dbg_triad", C.c_int, [C.c_int32, C.c_int64, C.c_int32, _P]),
    ("pt_dbg_valu_rate", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("pt_last_counters", C.c_int, [_P, _P]),
    ("pt_dbg_trace_timeline", C.c_int, [_P, _P, C.c_int32]),
    ("pt_enable_counters", C.c_int, [_P, C.c_int32]),
    ("pt_set_mode", C.c_int, [_P, C.c_int32]),
    ("pt_enable_trace_timing", C.c_int, [_P, C.c_int32]),
    ("pt_trace_timing", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    ("pt_shade_timing", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    ("pt_last_iterations", C.c_int, [_P]),
    ("pt_set_drain_threshold", C.c_int, [_P, C.c_int32]),
    ("pt_set_shade_rounds", C.c_int, [_P, C.c_int32]),
    ("pt_set_early_shade", C.c_int, [_P, C.c_int32]),
    ("pt_aov_floats", C.c_int64, [C.POINTER(PtCamera)]),
    ("pt_render_aov", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), _P, _P, _P]),
    ("pt_aov", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), _P, _P]),
    ("pt_denoise_params_default", None, [C.POINTER(PtDenoiseParams)]),
    ("pt_denoise_work_bytes", C.c_int64, [C.c_int32, C.c_int32]),
    ("pt_denoise", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PtDenoiseParams), _P, _P, _P]),
    ("pt_denoise_host", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PtDenoiseParams), _P]),
    ("pt_aov_window_floats", C.c_int64, [C.POINTER(PtCamera), C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("pt_render_aov_window", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pt_aov_window", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("pt_aov_views_floats", C.c_int64, [C.POINTER(PtCamera), C.c_int32]),
    ("pt_render_aov_views", C.c_int, [_P, C.POINTER(PtCamera), C.c_int32, C.POINTER(PtParams), _P, _P, _P, _P]),
    ("pt_aov_views", C.c_int, [_P, C.POINTER(PtCamera), C.c_int32, C.POINTER(PtParams), _P, _P, _P]),
    ("pt_aov_rays", C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    ("pt_aov_rays_host", C.c_int, [_P, _P, C.c_int64, _P, _P]),
    ("pt_untile_views", C.c_int, [_P, C.POINTER(PtCamera), C.c_int32, _P, _P]),
    ("pt_denoise_batch_work_bytes", C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    ("pt_denoise_batch", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PtDenoiseParams), _P, _P, _P]),
    ("pt_denoise_batch_host", C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PtDenoiseParams), _P]),
    ("pt_denoise_margin", C.c_int32, [C.c_int32]),
    ("pt_window_expand", C.c_int, [C.POINTER(PtCamera), C.POINTER(C.c_int32 * 4), C.c_int32, C.POINTER(C.c_int32 * 4)]),
    ("pt_accumulate_passes", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), C.c_int32, _P, _P, _P]),
    ("pt_variance", C.c_int, [_P, C.c_int64, C.c_int32, _P, _P]),
    ("pt_error_scratch_bytes", C.c_int64, [C.c_int64]),
    ("pt_error_estimate", C.c_int, [_P, _P, C.POINTER(PtCamera), C.POINTER(PtParams), C.c_int32, _P, C.POINTER(PtErrorEstimate), _P]),
    ("pt_render_converge", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), C.c_double, C.c_int32, _P, _P, C.POINTER(C.c_int32),
                                     C.POINTER(PtErrorEstimate)]),
    ("pt_accumulate_tile_list", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("pt_tile_errors", C.c_int, [_P, _P, C.POINTER(PtCamera), _P, C.c_int32, C.c_int32, _P, _P]),
    ("pt_finish_tiles", C.c_int, [_P, _P, _P, C.POINTER(PtCamera), _P, _P, _P]),
    ("pt_render_adaptive", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), C.c_double, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                     C.POINTER(PtAdaptiveReport)]),
    ("pt_tile_list_floats", C.c_int64, [C.c_int32]),
    ("pt_tile_list_work_bytes", C.c_int64, [C.POINTER(PtCamera), C.POINTER(PtParams), C.c_int32]),
    ("pt_render_tile_list", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), _P, C.c_int32, _P, _P, _P]),
    ("pt_tiles_of_window", C.c_int32, [C.POINTER(PtCamera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    ("pt_untile_list", C.c_int, [_P, _P, C.c_int32, C.POINTER(PtCamera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    ("pt_render_window", C.c_int, [_P, C.POINTER(PtCamera), C.POINTER(PtParams), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("pt_views_floats", C.c_int64, [C.POINTER(PtCamera), C.c_int32]),
    ("pt_views_work_bytes", C.c_int64, [C.POINTER(PtCamera), C.POINTER(PtParams), C.c_int32]),
    ("pt_render_views", C.c_int, [_P, C.POINTER(PtCamera), C.c_int32, C.POINTER(PtParams), _P, _P, _P, _P]),
    ("pt_render_views_host", C.c_int, [_P, C.POINTER(PtCamera), C.c_int32, C.POINTER(PtParams), _P, _P]),
    ("pt_scene_update_vertices", C.c_int, [_P, _P, _P, _P]),
    ("pt_scene_update_vertices_host", C.c_int, [_P, _P, _P]),
    ("pt_scene_update_spheres", C.c_int, [_P, _P, C.c_int32]),
    ("pt_scene_tree_inflation", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("pt_dbg_scene_array", C.c_int64, [_P, C.c_int32, _P, C.c_int64]),
    ("pt_scene_rebuild_tree", C.c_int, [_P, _P]),
    ("pt_scene_tree_info", C.c_int, [_P, C.POINTER(PtTreeInfo)]),
    ("pt_rebuild_params_default", None, [C.POINTER(PtRebuildParams)]),
    ("pt_scene_rebuild_tree_ex", C.c_int, [_P, C.POINTER(PtRebuildParams), C.POINTER(PtRebuildReport), _P]),
    ("pt_rebuild_opt_passes_default", C.c_int32, []),
    ("pt_scene_rebuild_tree_opt", C.c_int, [_P, C.POINTER(PtRebuildParams), C.c_int32, C.POINTER(PtRebuildOptReport), _P]),
    ("pt_dbg_tree_limits", C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("pt_scene_update_materials", C.c_int, [_P, _P, _P]),
    ("pt_scene_update_materials_host", C.c_int, [_P, _P]),
    ("pt_scene_update_sphere_materials", C.c_int, [_P, _P, C.c_int32]),
    ("pt_scene_nee_prune", C.c_int32, [_P]),
    ("pt_trace_rays", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    ("pt_trace_rays_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    ("pt_closest_points", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    ("pt_closest_points_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    ("pt_nearest_k", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    ("pt_nearest_k_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    ("pt_count_within", C.c_int, [_P, _P, C.c_int64, _P, _P]),
    ("pt_count_within_host", C.c_int, [_P, _P, C.c_int64, _P]),
    ("pt_trace_rays_k", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P]),
    ("pt_trace_rays_k_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    ("pt_count_hits", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    ("pt_count_hits_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    ("pt_list_offsets_scratch_bytes", C.c_int64, [C.c_int64]),
    ("pt_list_offsets", C.c_int, [_P, C.c_int64, _P, _P, _P]),
    ("pt_trace_rays_list", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, _P, _P, _P]),
    ("pt_within_radius_list", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P, _P]),
    ("pt_trace_rays_list_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, _P, _P]),
    ("pt_within_radius_list_host", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("pt_query_filter_default", None, [C.POINTER(PtQueryFilter)]),
    ("pt_trace_rays_f", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_trace_rays_k_f", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_count_hits_f", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_trace_rays_list_f", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_closest_points_f", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_nearest_k_f", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_count_within_f", C.c_int, [_P, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_within_radius_list_f", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_box_count", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_box_any", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_box_list", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_box_count_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    ("pt_box_any_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    ("pt_box_list_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int64, _P]),
    ("pt_convex_count", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_convex_any", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_convex_list", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_convex_count_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    ("pt_convex_any_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    ("pt_convex_list_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    ("pt_camera_frustum", C.c_int, [C.POINTER(PtCamera), C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    ("pt_sweep_spheres", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_sweep_spheres_host", C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    ("pt_tri_count", C.c_int, [_P, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_tri_any", C.c_int, [_P, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P]),
    ("pt_tri_list", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(PtQueryFilter), _P, _P, _P]),
    ("pt_tri_count_host", C.c_int, [_P, _P, C.c_int64, _P]),
    ("pt_tri_any_host", C.c_int, [_P, _P, C.c_int64, _P]),
    ("pt_tri_list_host", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    ("pt_rays_floats", C.c_int64, [C.c_int64]),
    ("pt_rays_work_bytes", C.c_int64, [C.POINTER(PtParams), C.c_int64]),
    ("pt_render_rays", C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.POINTER(PtParams), _P, _P, _P]),
    ("pt_render_rays_host", C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.POINTER(PtParams), _P]),
]

# pt_dbg_scene_array: name -> (which, dtype of the download)
SCENE_ARRAYS = {"nodes": (0, np.float32), "quad": (1, np.uint32), "tri": (2, np.float32), "tripair": (3, np.float32), "leafbox": (4, np.float32),
                "surf": (5, np.float32), "lights": (6, np.float32), "spheres": (7, np.float32), "core": (8, np.float32)}


def lib():
    """Load libptamd.so (built by __graft_entry__.build() / `make -C pathtrace-on-cuda_amd`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PtError(f"{LIB_PATH} is missing: build it with `make -C {PKG_ROOT}` "
                          "(there is no CPU fallback for the render path)")
        # torch, where it is installed, has to meet the HIP runtime first.  Its libtorch_hip.so asks for "libamdhip64.so" by that bare
        # name, with an RPATH to the copy torch ships, whose SONAME is libamdhip64.so.N; libptamd.so asks for libamdhip64.so.N.  With
        # torch loaded first the loader satisfies libptamd.so by SONAME from torch's copy: one runtime in the process.  The other way
        # round ROCm's copy is loaded, the bare name matches no loaded SONAME, torch opens its own copy beside it, and that second
        # runtime finds no GPU ("No HIP GPUs are available") — in every call that stages numpy through torch (QueryFilter,
        # list_offsets) after a Scene exists.  Importing torch initialises no device.
        if "torch" not in sys.modules:
            try:
                import torch      # noqa: F401
            except ImportError:
                pass              # no torch: the C-ABI paths need none, and the ones that do say so when they import it
        l = C.CDLL(LIB_PATH)
        for name, res, args in API:
            fn = getattr(l, name)       # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def _check(rc, what):
    if rc != 0:
        raise PtError(f"{what} failed ({rc}): {lib().pt_last_error().decode()}")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _device_points(who, points, device):
    """The host-side checks of a POINT4 tensor for the scene on `device`; returns n."""
    if not (hasattr(points, "data_ptr") and hasattr(points, "is_contiguous")):
        raise PtError(f"{who}: points must be a torch tensor or a numpy array")
    if str(points.dtype) != "torch.float32" or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 4:
        raise PtError(f"{who}: points must be contiguous float32 of shape (n, 4), got {points.dtype} {tuple(points.shape)}")
    if points.device.type != "cuda" or points.device.index != device:
        raise PtError(f"{who}: points is on {points.device}, the scene is on device {device}")
    return points.shape[0]


def _device_rays(who, rays, device):
    """The host-side checks of a RAY8 tensor for the scene on `device`; returns n."""
    if not (hasattr(rays, "data_ptr") and hasattr(rays, "is_contiguous")):
        raise PtError(f"{who}: rays must be a torch tensor or a numpy array")
    if str(rays.dtype) != "torch.float32" or not rays.is_contiguous() or rays.dim() != 2 or rays.shape[1] != 8:
        raise PtError(f"{who}: rays must be contiguous float32 of shape (n, 8), got {rays.dtype} {tuple(rays.shape)}")
    if rays.device.type != "cuda" or rays.device.index != device:
        raise PtError(f"{who}: rays is on {rays.device}, the scene is on device {device}")
    return rays.shape[0]


def _device_sweeps(who, sweeps, device):
    """The host-side checks of a SWEEP8 tensor for the scene on `device`; returns n."""
    if not (hasattr(sweeps, "data_ptr") and hasattr(sweeps, "is_contiguous")):
        raise PtError(f"{who}: sweeps must be a torch tensor or a numpy array")
    if str(sweeps.dtype) != "torch.float32" or not sweeps.is_contiguous() or sweeps.dim() != 2 or sweeps.shape[1] != 8:
        raise PtError(f"{who}: sweeps must be contiguous float32 of shape (n, 8), got {sweeps.dtype} {tuple(sweeps.shape)}")
    if sweeps.device.type != "cuda" or sweeps.device.index != device:
        raise PtError(f"{who}: sweeps is on {sweeps.device}, the scene is on device {device}")
    return sweeps.shape[0]


def _device_tris(who, tris, device):
    """The checks of a query's device path on TRI12 records, (n, 12) float32: n."""
    if not (hasattr(tris, "data_ptr") and hasattr(tris, "is_contiguous")):
        raise PtError(f"{who}: tris must be a torch tensor or a numpy array")
    if str(tris.dtype) != "torch.float32" or not tris.is_contiguous() or tris.dim() != 2 or tris.shape[1] != 12:
        raise PtError(f"{who}: tris must be contiguous float32 of shape (n, 12), got {tris.dtype} {tuple(tris.shape)}")
    if tris.device.type != "cuda" or tris.device.index != device:
        raise PtError(f"{who}: tris is on {tris.device}, the scene is on device {device}")
    return tris.shape[0]


def _device_boxes(who, boxes, device):
    """The host-side checks of a BOX8 tensor for the scene on `device`; returns n."""
    if not (hasattr(boxes, "data_ptr") and hasattr(boxes, "is_contiguous")):
        raise PtError(f"{who}: boxes must be a torch tensor or a numpy array")
    if str(boxes.dtype) != "torch.float32" or not boxes.is_contiguous() or boxes.dim() != 2 or boxes.shape[1] != 8:
        raise PtError(f"{who}: boxes must be contiguous float32 of shape (n, 8), got {boxes.dtype} {tuple(boxes.shape)}")
    if boxes.device.type != "cuda" or boxes.device.index != device:
        raise PtError(f"{who}: boxes is on {boxes.device}, the scene is on device {device}")
    return boxes.shape[0]


def _host_rows(who, a, name, width):
    """The numpy path of a query: `a` as contiguous float32 rows of `width` floats; returns (array, n)."""
    x = np.ascontiguousarray(a, np.float32)
    if x.ndim != 2 or x.shape[1] != width:
        raise PtError(f"{who}: {name} has shape {x.shape}, want (n, {width})")
    return x, x.shape[0]


def _host_out(shape, dtype, detail, det_width):
    """The numpy outputs of a query: zeroed records of the tuple `shape` and, if detail, zeroed float32 detail records of
    shape + (det_width,), else None."""
    return np.zeros(shape, dtype), (np.zeros(shape + (det_width,), np.float32) if detail else None)


def _records(res, det):
    """A query's result from its 8-byte records: (key, prim), float32 and int32, and det as a third item unless it is None.  res: a
    numpy structured array (HIT_DTYPE, NEAREST_DTYPE) or an int32 torch tensor of shape (..., 2) (key's bits | prim)."""
    if isinstance(res, np.ndarray):
        out = tuple(np.ascontiguousarray(res[f]) for f in res.dtype.names)
    else:
        import torch
        out = (res[..., 0].view(torch.float32), res[..., 1])
    return out if det is None else out + (det,)


def _csr(who, a, name, width, dtype, det_width, detail, stream_ptr, device, device_rows, count, host_list, device_list):
    """The CSR routine of Scene.trace_rays_all and Scene.within_radius on the scene on `device`.  a: the queries, rows of `width`
    floats (device_rows: their device-side checks); count(a): the per-query counts on the device; host_list / device_list(a, n,
    offsets, cap, records, detail): the list's _host and device entry points, checked, with pointers.  The numpy path makes the
    sizing call, then the fill; the device path counts, scans, reads the total back and fills, on stream_ptr."""
    if isinstance(a, np.ndarray):
        x, n = _host_rows(who, a, name, width)
        off = np.zeros(n + 1, np.int64)
        host_list(_ptr(x), n, _ptr(off), 0, None, None)
        total = int(off[n])
        res, det = _host_out((total,), dtype, detail, det_width)
        if total:
            host_list(_ptr(x), n, _ptr(off), total, _ptr(res), _ptr(det) if detail else None)
        return (off,) + _records(res, det)
    n = device_rows(who, a, device)
    import torch
    if n == 0:
        off, total = torch.zeros(1, dtype=torch.int64, device=a.device), 0
    else:
        off = list_offsets(count(a), stream_ptr=stream_ptr)
        total = _read_total(off, stream_ptr)
    res = torch.empty((total, 2), dtype=torch.int32, device=a.device)      # PtRayHit / PtNearest: key's bits | prim
    det = torch.empty((total, det_width), dtype=torch.float32, device=a.device) if detail else None
    if total:
        device_list(C.c_void_p(a.data_ptr()), n, C.c_void_p(off.data_ptr()), total, C.c_void_p(res.data_ptr()),
                    C.c_void_p(det.data_ptr()) if detail else None)
    return (off,) + _records(res, det)


class QueryFilter:
    """Which primitives a query may answer with (include/pt_api.h: "Query filters"): the `filter=` argument of Scene.trace_rays,
    trace_rays_k, count_hits, trace_rays_all, closest_points, nearest_k, count_within and within_radius.
      prim_bits   one 32-bit word per primitive (triangles in the order of `tris`, then spheres); None: every bit set
      query_bits  one word per ray / point; None: `bits` for every query
      skip        one int32 per ray / point, the primitive that query ignores (-1, or anything that is no primitive: none); None: none
      tmin        True (ray queries only): the 7th float of each ray is its near bound; a hit at exactly tmin is kept
    A primitive is a member for query i iff (prim_bits[prim] & query_bits[i]) != 0 and prim != skip[i].  The arrays are contiguous 1-D
    torch tensors (int32 or uint32) on the scene's device, used in place, or numpy arrays (uint32 / int32), which are uploaded with
    torch to the scene's device at their first use and kept.  The filter keeps its arrays alive; they must not change while a query
    that reads them is in flight."""

    def __init__(self, prim_bits=None, bits=0xFFFFFFFF, query_bits=None, skip=None, tmin=False):
        bits = int(bits)
        if not 0 <= bits <= 0xFFFFFFFF:
            raise PtError(f"QueryFilter: bits = {bits:#x} is not a 32-bit word")
        self.bits, self.tmin = bits, bool(tmin)
        self._given = {"prim_bits": self._checked("prim_bits", prim_bits, ("uint32", "int32")),
                       "query_bits": self._checked("query_bits", query_bits, ("uint32", "int32")),
                       "skip": self._checked("skip", skip, ("int32",))}
        self._on = {}      # device -> {name: torch tensor there}

    @staticmethod
    def _checked(name, a, dtypes):
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            if a.ndim != 1 or a.dtype.name not in dtypes:
                raise PtError(f"QueryFilter: {name} must be a 1-D array of {' or '.join(dtypes)}, got {a.dtype} {a.shape}")
            return np.ascontiguousarray(a)
        if not (hasattr(a, "data_ptr") and hasattr(a, "is_contiguous")):
            raise PtError(f"QueryFilter: {name} must be a torch tensor or a numpy array")
        if str(a.dtype).replace("torch.", "") not in dtypes or a.dim() != 1 or not a.is_contiguous():
            raise PtError(f"QueryFilter: {name} must be a contiguous 1-D tensor of {' or '.join(dtypes)}, got {a.dtype} {tuple(a.shape)}")
        return a

    def _checks(self, who, device, n, n_prims, rays):
        """This filter's checks for n queries of the scene on `device` with n_prims primitives: no device call."""
        if self.tmin and not rays:
            raise PtError(f"{who}: tmin applies to ray queries only")
        for name, want in (("prim_bits", n_prims), ("query_bits", n), ("skip", n)):      # every check before the first upload
            a = self._given[name]
            if a is None:
                continue
            if a.shape[0] != want:
                raise PtError(f"{who}: filter {name} has {a.shape[0]} entries, want {want}")
            if not isinstance(a, np.ndarray) and (a.device.type != "cuda" or a.device.index != device):
                raise PtError(f"{who}: filter {name} is on {a.device}, the scene is on device {device}")

    def _bind(self, who, device, n, n_prims, rays):
        """The PtQueryFilter of this filter, after _checks of the same arguments; uploads what is numpy."""
        self._checks(who, device, n, n_prims, rays)
        on = self._on.setdefault(device, {})
        ptr = {}
        for name, a in self._given.items():
            if isinstance(a, np.ndarray):
                if name not in on:
                    import torch
                    on[name] = torch.from_numpy(a.view(np.int32)).to(f"cuda:{device}")
                a = on[name]
            ptr[name] = (a.data_ptr() or None) if a is not None else None
        return PtQueryFilter(ptr["prim_bits"], ptr["query_bits"], ptr["skip"], self.bits, FILTER_TMIN if self.tmin else 0)

    def struct(self, scene, n, rays=False):
        """The PtQueryFilter of this filter for n queries (rays, else points or boxes) of `scene`, for a caller who passes it to the
        C-ABI directly (C.byref(...)): checked as the Scene methods check it; numpy arrays are uploaded at their first use.  The filter
        must outlive the calls that read the struct."""
        return self._bind("QueryFilter.struct", scene.device, int(n), scene.n_tris + scene.n_spheres, bool(rays))


def _rebuild_params(depth_budget, large_fraction):
    """PtRebuildParams of the two optional arguments of Scene.rebuild_tree / rebuild_tree_optimized: a None takes its default."""
    prm = PtRebuildParams()
    lib().pt_rebuild_params_default(C.byref(prm))
    if depth_budget is not None:
        prm.depth_budget = depth_budget
    if large_fraction is not None:
        prm.large_fraction = large_fraction
    return prm


def default_params(**kw):
    p = PtParams()
    lib().pt_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def camera_basis(rot_deg=(0.0, 90.0, 0.0)):
    r = (C.c_float * 3)(*rot_deg)
    f, u, rt = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
    lib().pt_camera_basis(C.byref(r), C.byref(f), C.byref(u), C.byref(rt))
    return np.array(f[:], np.float32), np.array(u[:], np.float32), np.array(rt[:], np.float32)


def make_camera(W, H, pos=(0.0, 20.0, 60.0), rot_deg=(0.0, 90.0, 0.0), fovy_deg=45.0):
    """The reference app's camera: Renderer ctor puts it at (0,20,60) with rotation (0,90,0)
    (srcs/renderer.cpp:28-30); SetScreenSize sets aspect = W/H (srcs/renderer.cpp:47-53)."""
    f, u, r = camera_basis(rot_deg)
    c = PtCamera()
    c.pos[:] = pos
    c.forward[:] = f.tolist()
    c.up[:] = u.tolist()
    c.right[:] = r.tolist()
    c.fovy_deg = fovy_deg
    c.aspect = np.float32(W) / np.float32(H)
    c.W, c.H = W, H
    return c


def gen_scene(kind, lat_lon=187):
    """Procedural scene as a (n, 84) float32 array of reference `Primitive` records."""
    n = lib().pt_scene_gen(kind, lat_lon, None, 0)
    if n < 0:
        _check(n, "pt_scene_gen")
    prims = np.zeros((n, PRIM_FLOATS), np.float32)
    n2 = lib().pt_scene_gen(kind, lat_lon, _ptr(prims), n)
    assert n2 == n
    return prims


def build_bvh(prims):
    """SAH build + flatten.  Returns (nodes[NODE_DTYPE], tris float32 (n,88), max_depth)."""
    prims = np.ascontiguousarray(prims, np.float32)
    assert prims.ndim == 2 and prims.shape[1] == PRIM_FLOATS
    h = C.c_void_p()
    _check(lib().pt_bvh_build_sah(_ptr(prims), prims.shape[0], C.byref(h)), "pt_bvh_build_sah")
    try:
        nn, nt = lib().pt_bvh_num_nodes(h), lib().pt_bvh_num_tris(h)
        nodes = np.frombuffer(C.string_at(lib().pt_bvh_nodes(h), nn * NODE_BYTES), NODE_DTYPE).copy()
        tris = np.frombuffer(C.string_at(lib().pt_bvh_tris(h), nt * TRI_FLOATS * 4), np.float32).reshape(nt, TRI_FLOATS).copy()
        depth = lib().pt_bvh_max_depth(h)
    finally:
        lib().pt_bvh_free(h)
    return nodes, tris, depth


def make_sphere(center, rad, emittance=(0, 0, 0), albedo=(1, 1, 1), specular=(0.04, 0.04, 0.04),
                opacity=1.0, roughness=0.2, metallic=1.0):
    """One PtSphere record (16 float32): center rad | emittance albedo specular opacity roughness metallic."""
    return np.array([*center, rad, *emittance, *albedo, *specular, opacity, roughness, metallic], np.float32)


def tonemap_u8(raw_rgb, sample_cnt):
    raw = np.ascontiguousarray(raw_rgb, np.float32)
    out = np.zeros(raw.shape, np.uint8)
    _check(lib().pt_tonemap_u8(_ptr(raw), raw.size // 3, sample_cnt, _ptr(out)), "pt_tonemap_u8")
    return out


def convert_u8(values):
    """ConverToUint8 (include/image.h:5-8), element-wise."""
    v = np.ascontiguousarray(values, np.float32)
    out = np.zeros(v.shape, np.uint8)
    _check(lib().pt_convert_u8(_ptr(v), v.size, _ptr(out)), "pt_convert_u8")
    return out


def write_png(path, rgb8):
    a = np.ascontiguousarray(rgb8, np.uint8)
    H, W, ch = a.shape
    _check(lib().pt_write_png(path.encode(), _ptr(a), W, H, ch), "pt_write_png")


class Scene:
    """An uploaded scene (PtScene): HBM-resident wide-node BVH, triangle records, lights."""

    def __init__(self, nodes, tris, spheres=None, device=0):
        nodes = np.ascontiguousarray(nodes)
        tris = np.ascontiguousarray(tris, np.float32)
        assert nodes.dtype == NODE_DTYPE and tris.ndim == 2 and tris.shape[1] == TRI_FLOATS
        if spheres is None:
            spheres = np.zeros((0, SPHERE_FLOATS), np.float32)
        spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, SPHERE_FLOATS)
        self.device = device
        self.n_tris = tris.shape[0]
        self.n_spheres = spheres.shape[0]
        self._h = C.c_void_p()
        _check(lib().pt_scene_create(_ptr(nodes), nodes.shape[0], _ptr(tris), tris.shape[0],
                                     _ptr(spheres) if spheres.shape[0] else None, spheres.shape[0], device, C.byref(self._h)),
               "pt_scene_create")

    @classmethod
    def from_prims(cls, prims, spheres=None, device=0):
        nodes, tris, _ = build_bvh(prims)
        return cls(nodes, tris, spheres, device)

    def close(self):
        if self._h:
            lib().pt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def num_lights(self):
        return lib().pt_scene_num_lights(self._h)

    @property
    def device_bytes(self):
        return lib().pt_scene_device_bytes(self._h)

    def render(self, cam, prm):
        """Whole frame, synchronous; returns (H, W, 3) float32 accumulated radiance."""
        out = np.zeros((cam.H, cam.W, 3), np.float32)
        _check(lib().pt_render(self._h, C.byref(cam), C.byref(prm), _ptr(out)), "pt_render")
        return out

    def render_tiles(self, cam, prm, d_tiles_ptr, d_work_ptr, stream_ptr=0):
        """Device-resident render of this rank's tiles (raw device pointers), enqueued on the given stream; blocks until the
        render has drained in the default mode 1 (include/pt_api.h: pt_render_tiles)."""
        _check(lib().pt_render_tiles(self._h, C.byref(cam), C.byref(prm), C.c_void_p(d_tiles_ptr), C.c_void_p(d_work_ptr),
                                     C.c_void_p(stream_ptr)), "pt_render_tiles")

    def last_render_ms(self):
        ms = C.c_float()
        _check(lib().pt_last_render_ms(self._h, C.byref(ms)), "pt_last_render_ms")
        return ms.value

    def render_timings(self, reset=True):
        """ms of each recent render_units launch (HIP events on the launch stream)."""
        out = np.zeros(64, np.float32)
        n = lib().pt_render_timings(self._h, _ptr(out), 64, 1 if reset else 0)
        if n < 0:
            _check(n, "pt_render_timings")
        return out[:n].copy()

    def set_mode(self, mode):
        """1 = wavefront pipeline (default), 0 = one-kernel state machine."""
        _check(lib().pt_set_mode(self._h, mode), "pt_set_mode")

    def enable_trace_timing(self, max_launches=8192):
        _check(lib().pt_enable_trace_timing(self._h, max_launches), "pt_enable_trace_timing")

    def trace_timing(self):
        """(sum_ms, launches, max_ms) of the wf_trace launches of the last render (HIP events)."""
        s, n, m = C.c_double(), C.c_int32(), C.c_double()
        _check(lib().pt_trace_timing(self._h, C.byref(s), C.byref(n), C.byref(m)), "pt_trace_timing")
        return s.value, n.value, m.value

    def shade_timing(self):
        """(sum_ms, launches, max_ms) of the wf_shade launches of the last render (HIP events on the launch stream)."""
        s, n, m = C.c_double(), C.c_int32(), C.c_double()
        _check(lib().pt_shade_timing(self._h, C.byref(s), C.byref(n), C.byref(m)), "pt_shade_timing")
        return s.value, n.value, m.value

    def set_drain_threshold(self, live_streams):
        _check(lib().pt_set_drain_threshold(self._h, live_streams), "pt_set_drain_threshold")

    def set_early_shade(self, live_streams):
        """wf_shade starts beside the draining wf_trace while at most this many streams are alive (0 = never).  Result-neutral."""
        _check(lib().pt_set_early_shade(self._h, live_streams), "pt_set_early_shade")

    def set_shade_rounds(self, mode):
        """1: next sample starts in the step a path ends; 0: one bounce per step; -1: by live-stream count (result-neutral)."""
        _check(lib().pt_set_shade_rounds(self._h, mode), "pt_set_shade_rounds")

    def last_iterations(self):
        return lib().pt_last_iterations(self._h)

    def enable_counters(self, on=True):
        _check(lib().pt_enable_counters(self._h, 1 if on else 0), "pt_enable_counters")

    def counters(self):
        out = np.zeros(8, np.int64)
        _check(lib().pt_last_counters(self._h, _ptr(out)), "pt_last_counters")
        return out

    def trace_timeline(self, n_launches):
        """Diagnostic (PTAMD_TSTAT=1): per wf_trace launch (start, queue-empty, end) in 100 MHz ticks; 0 = not recorded."""
        raw = np.zeros((int(n_launches), 3), np.int64)
        _check(lib().pt_dbg_trace_timeline(self._h, _ptr(raw), int(n_launches)), "pt_dbg_trace_timeline")
        out = raw.copy()
        out[:, 0] = np.where(raw[:, 0] != 0, ~raw[:, 0], 0)
        out[:, 1] = np.where(raw[:, 1] != 0, ~raw[:, 1], 0)
        return out

    def trace_depth_hist(self):
        """Diagnostic (PTAMD_TSTAT=1): over the wf_trace launches of the last render, how many node steps left the ray's traversal stack
        with 0 .. 30 and with 31 or more entries (32 x int64).  Entries 16 and up lie in the stack's global-memory overflow."""
        raw = np.zeros(32, np.int64)
        _check(lib().pt_dbg_trace_timeline(self._h, _ptr(raw), -3001), "pt_dbg_trace_timeline")
        return raw

    def trace_step_hist(self):
        """Diagnostic (PTAMD_TSTAT=1): node steps per finished ray over the wf_trace launches of the last render, 64 bins of 4 steps
        (the last bin: 252 or more)."""
        raw = np.zeros(64, np.int64)
        _check(lib().pt_dbg_trace_timeline(self._h, _ptr(raw), -3000), "pt_dbg_trace_timeline")
        return raw

    def nee(self, in5):
        """pt_dbg_nee: rows of (p.xyz, seed lo, seed hi as uint32 bits) -> (n, 12) float32 (see include/pt_api.h)."""
        a = np.ascontiguousarray(in5, np.float32).reshape(-1, 5)
        out = np.zeros((a.shape[0], 12), np.float32)
        _check(lib().pt_dbg_nee(self._h, _ptr(a), a.shape[0], _ptr(out)), "pt_dbg_nee")
        return out

    def trace_launch_rays(self, n_launches):
        """Diagnostic (PTAMD_TSTAT=1 or 2): rays traced by each of the first n wf_trace launches of the last render."""
        raw = np.zeros(int(n_launches), np.int64)
        _check(lib().pt_dbg_trace_timeline(self._h, _ptr(raw), -int(n_launches)), "pt_dbg_trace_timeline")
        return raw

    def aov(self, cam, prm):
        """First-hit feature buffers of the passes prm.first_pass .. + prm.passes - 1 (include/pt_api.h: pt_render_aov), synchronous:
        ((H, W, 8) float32 albedo.rgb | normal.xyz | depth | coverage, (H, W) int32 primitive of the first pass's ray, -1 = miss)."""
        out = np.zeros((cam.H, cam.W, AOV_FLOATS), np.float32)
        prim = np.zeros((cam.H, cam.W), np.int32)
        _check(lib().pt_aov(self._h, C.byref(cam), C.byref(prm), _ptr(out), _ptr(prim)), "pt_aov")
        return out, prim

    def render_aov(self, cam, prm, d_aov_ptr, d_prim_ptr=0, stream_ptr=0):
        """Device-resident pt_render_aov into raw device pointers (d_prim_ptr 0 = none), enqueued on the given stream."""
        _check(lib().pt_render_aov(self._h, C.byref(cam), C.byref(prm), C.c_void_p(d_aov_ptr), C.c_void_p(d_prim_ptr or None),
                                   C.c_void_p(stream_ptr)), "pt_render_aov")

    def aov_window(self, cam, prm, window):
        """The feature buffers of the pixel window (x0, y0, x1, y1), half-open, synchronous (include/pt_api.h: pt_render_aov_window):
        ((y1 - y0, x1 - x0, 8) float32, (y1 - y0, x1 - x0) int32), bit for bit aov(cam, prm)[...][y0:y1, x0:x1]."""
        x0, y0, x1, y1 = (int(v) for v in window)
        out = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0), AOV_FLOATS), np.float32)
        prim = np.zeros(out.shape[:2], np.int32)
        _check(lib().pt_aov_window(self._h, C.byref(cam), C.byref(prm), x0, y0, x1, y1, _ptr(out), _ptr(prim)), "pt_aov_window")
        return out, prim

    def render_aov_window(self, cam, prm, window, d_aov_ptr, d_prim_ptr=0, stream_ptr=0):
        """Device-resident pt_render_aov_window into raw device pointers (aov_window_floats(cam, window) floats; d_prim_ptr 0 = none),
        enqueued on the given stream; nothing is allocated and nothing read back."""
        x0, y0, x1, y1 = (int(v) for v in window)
        _check(lib().pt_render_aov_window(self._h, C.byref(cam), C.byref(prm), x0, y0, x1, y1, C.c_void_p(d_aov_ptr), C.c_void_p(d_prim_ptr or None),
                                          C.c_void_p(stream_ptr)), "pt_render_aov_window")

    def aov_views(self, cams, prm, first_pass=None):
        """The feature buffers of a batch of cameras of one size in one launch, synchronous (include/pt_api.h: pt_render_aov_views):
        ((V, H, W, 8) float32, (V, H, W) int32), [v] bit for bit aov(cams[v], prm) (with first_pass[v] as its first pass where given)."""
        arr = _camera_array(cams)
        fp = _first_passes(first_pass, len(arr))
        out = np.zeros((len(arr), arr[0].H, arr[0].W, AOV_FLOATS), np.float32)
        prim = np.zeros(out.shape[:3], np.int32)
        _check(lib().pt_aov_views(self._h, arr, len(arr), C.byref(prm), _ptr(fp) if fp is not None else None, _ptr(out), _ptr(prim)), "pt_aov_views")
        return out, prim

    def render_aov_views(self, cams, prm, d_aov_ptr, d_prim_ptr=0, stream_ptr=0, first_pass=None):
        """Device-resident pt_render_aov_views into raw device pointers (aov_views_floats(cams[0], n) floats, view-major; d_prim_ptr 0 =
        none).  Waits for the stream once (the camera table's upload); the kernel is asynchronous on it."""
        arr = _camera_array(cams)
        fp = _first_passes(first_pass, len(arr))
        _check(lib().pt_render_aov_views(self._h, arr, len(arr), C.byref(prm), _ptr(fp) if fp is not None else None, C.c_void_p(d_aov_ptr),
                                         C.c_void_p(d_prim_ptr or None), C.c_void_p(stream_ptr)), "pt_render_aov_views")

    def aov_rays(self, rays, stream_ptr=0):
        """The feature buffers of the caller's rays (include/pt_api.h: pt_aov_rays).  rays: (n, 8) float32 RAY8 records as in trace_rays.
        Returns ((n, 8) float32 albedo.rgb | normal.xyz | t | 1, zeros for a miss, and (n,) int32 primitive, -1 = miss).  A torch float32
        tensor on the scene's device is used in place (data_ptr()): the call is enqueued on stream_ptr, the results are torch tensors on
        that device, valid once the stream has passed it, and `rays` must stay alive until then.  A numpy array goes through
        pt_aov_rays_host (synchronous) and returns numpy arrays."""
        if isinstance(rays, np.ndarray):
            r = np.ascontiguousarray(rays, np.float32)
            if r.ndim != 2 or r.shape[1] != 8:
                raise PtError(f"aov_rays: rays has shape {r.shape}, want (n, 8)")
            n = r.shape[0]
            out, prim = np.zeros((n, AOV_FLOATS), np.float32), np.zeros(n, np.int32)
            _check(lib().pt_aov_rays_host(self._h, _ptr(r), n, _ptr(out), _ptr(prim)), "pt_aov_rays_host")
            return out, prim
        if not (hasattr(rays, "data_ptr") and hasattr(rays, "is_contiguous")):
            raise PtError("aov_rays: rays must be a torch tensor or a numpy array")
        if str(rays.dtype) != "torch.float32" or not rays.is_contiguous() or rays.dim() != 2 or rays.shape[1] != 8:
            raise PtError(f"aov_rays: rays must be contiguous float32 of shape (n, 8), got {rays.dtype} {tuple(rays.shape)}")
        if rays.device.type != "cuda" or rays.device.index != self.device:
            raise PtError(f"aov_rays: rays is on {rays.device}, the scene is on device {self.device}")
        import torch
        n = rays.shape[0]
        out = torch.empty((n, AOV_FLOATS), dtype=torch.float32, device=rays.device)
        prim = torch.empty(n, dtype=torch.int32, device=rays.device)
        self.aov_rays_device(rays.data_ptr(), n, out.data_ptr(), prim.data_ptr(), stream_ptr)
        return out, prim

    def aov_rays_device(self, d_rays_ptr, n_rays, d_aov_ptr, d_prim_ptr=0, stream_ptr=0):
        """pt_aov_rays on raw device pointers (d_prim_ptr 0 = none), enqueued on the given stream."""
        _check(lib().pt_aov_rays(self._h, C.c_void_p(d_rays_ptr), int(n_rays), C.c_void_p(d_aov_ptr), C.c_void_p(d_prim_ptr or None),
                                 C.c_void_p(stream_ptr)), "pt_aov_rays")

    def render_window_denoised(self, cam, prm, window, margin=None, **params):
        """The pixel window (x0, y0, x1, y1) of the denoised frame without the full frame: the window grown by `margin` (None: what the
        filter's iterations reach, denoise_margin — then the result is bit for bit denoise(render(cam, prm), aov(cam, prm)[0],
        prm.passes, **params)[y0:y1, x0:x1]) is rendered, its feature buffers are made, denoised and cropped.  Synchronous;
        (y1 - y0, x1 - x0, 3) float32.  A smaller margin is cheaper and makes no equality claim (include/pt_api.h: pt_window_expand)."""
        p = denoise_params(**params)
        x0, y0, x1, y1 = (int(v) for v in window)
        ex = expand_window(cam, (x0, y0, x1, y1), denoise_margin(p.iterations) if margin is None else int(margin))
        rgb = self.render_window(cam, prm, ex)
        aov, _ = self.aov_window(cam, prm, ex)
        out = denoise(rgb, aov, prm.passes, self.device, **params)
        return np.ascontiguousarray(out[y0 - ex[1]:y1 - ex[1], x0 - ex[0]:x1 - ex[0]])

    def render_views_denoised(self, cams, prm, first_pass=None, **params):
        """A batch of cameras of one size rendered and denoised on one stream with one download: render_views_device, untile_views,
        the feature buffers of the batch and denoise_batch.  (V, H, W, 3) float32, [v] bit for bit denoise(render(cams[v], ...),
        aov(cams[v], ...)[0], prm.passes, **params).  torch provides the device buffers."""
        import torch
        arr = _camera_array(cams)
        V, W, H = len(arr), arr[0].W, arr[0].H
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            tiles = torch.empty(views_floats(arr[0], V), dtype=torch.float32, device=dev)
            work = torch.empty(max(views_work_bytes(arr[0], prm, V), denoise_batch_work_bytes(W, H, V)), dtype=torch.uint8, device=dev)
            frames = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
            aov = torch.empty((V, H, W, AOV_FLOATS), dtype=torch.float32, device=dev)
            out = torch.empty_like(frames)
            st = torch.cuda.current_stream(dev).cuda_stream
            self.render_views_device(arr, prm, tiles.data_ptr(), work.data_ptr(), st, first_pass)
            untile_views(tiles.data_ptr(), arr[0], V, frames.data_ptr(), st)
            self.render_aov_views(arr, prm, aov.data_ptr(), 0, st, first_pass)
            denoise_batch_device(frames.data_ptr(), aov.data_ptr(), W, H, V, prm.passes, out.data_ptr(), work.data_ptr(), st, **params)
            return out.cpu().numpy()

    def render_stats(self, cam, prm):
        """Whole frame with its per-pixel variance across the call's passes (prm.passes >= 2), synchronous: one pt_render_tiles,
        pt_accumulate_passes, pt_variance and two pt_untile.  Returns ((H, W, 3) float32 frame — bit for bit what render()
        returns — and (H, W, 3) float32 estimated variance of it).  torch provides the device buffers."""
        import torch
        p = PtParams.from_buffer_copy(prm)
        p.rank, p.world = 0, 1
        n = tiles_floats(cam, p)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            tiles = torch.empty((3, n), dtype=torch.float32, device=dev)          # frame tiles | S | M2 (then the variance)
            work = torch.empty(work_bytes(cam, p), dtype=torch.uint8, device=dev)
            frames = torch.empty((2, cam.H, cam.W, 3), dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            self.render_tiles(cam, p, tiles[0].data_ptr(), work.data_ptr(), st)
            accumulate_passes(work.data_ptr(), cam, p, 0, tiles[1].data_ptr(), tiles[2].data_ptr(), st)
            variance(tiles[2].data_ptr(), n, p.passes, tiles[0].data_ptr(), st)
            untile(tiles[1].data_ptr(), cam, 1, frames[0].data_ptr(), st)
            untile(tiles[0].data_ptr(), cam, 1, frames[1].data_ptr(), st)
            out = frames.cpu().numpy()
        return out[0], out[1]

    def render_converge(self, cam, prm, target_rel_rms, max_passes):
        """pt_render_converge: batches of prm.passes passes until the estimated relative RMS error is <= target_rel_rms or
        max_passes are in.  Returns (frame (H, W, 3) float32 = the sum over passes_done passes, variance of it (H, W, 3),
        passes_done, dict(rel_rms, mean_rel_se, pixels, skipped))."""
        rgb = np.zeros((cam.H, cam.W, 3), np.float32)
        var = np.zeros((cam.H, cam.W, 3), np.float32)
        done, est = C.c_int32(0), PtErrorEstimate()
        _check(lib().pt_render_converge(self._h, C.byref(cam), C.byref(prm), float(target_rel_rms), int(max_passes), _ptr(rgb), _ptr(var),
                                        C.byref(done), C.byref(est)), "pt_render_converge")
        return rgb, var, done.value, _estimate_dict(est)

    def render_adaptive(self, cam, prm, target, max_passes, min_passes=2):
        """pt_render_adaptive: rounds of prm.passes passes over the tiles whose own error estimate (mean_rel_se over the tile's pixels)
        is still above `target`, checked once min_passes are in, until no tile is left or max_passes are in.  Returns a dict:
        rgb (H, W, 3) float32 = S, every tile the sum over ITS passes; mean (H, W, 3) = S / the tile's passes, the frame to show
        (tonemap_u8(mean, 1)); var (H, W, 3) = the variance of S; tile_passes (tiles_y, tiles_x) int32; tile_err (tiles_y, tiles_x)
        float64, the error at the tile's last check; report = dict(rounds, tiles, tiles_converged, tile_passes, max_tile_err)."""
        ty, tx = (cam.H + TILE - 1) // TILE, (cam.W + TILE - 1) // TILE
        rgb, mean, var = (np.zeros((cam.H, cam.W, 3), np.float32) for _ in range(3))
        tile_passes, tile_err = np.zeros((ty, tx), np.int32), np.zeros((ty, tx), np.float64)
        rep = PtAdaptiveReport()
        _check(lib().pt_render_adaptive(self._h, C.byref(cam), C.byref(prm), float(target), int(min_passes), int(max_passes), _ptr(rgb), _ptr(mean),
                                        _ptr(var), _ptr(tile_passes), _ptr(tile_err), C.byref(rep)), "pt_render_adaptive")
        report = dict(rounds=rep.rounds, tiles=rep.tiles, tiles_converged=rep.tiles_converged, tile_passes=rep.tile_passes,
                      max_tile_err=rep.max_tile_err)
        return dict(rgb=rgb, mean=mean, var=var, tile_passes=tile_passes, tile_err=tile_err, report=report)

    def render_tile_list_device(self, cam, prm, tiles, d_tiles_ptr, d_work_ptr, stream_ptr=0):
        """Device-resident render of the listed tiles (global tile numbers, any order; raw device pointers: tile_list_floats(n)
        floats, tile_list_work_bytes(cam, prm, n) bytes), enqueued on the given stream; blocks until the render has drained
        (include/pt_api.h: pt_render_tile_list)."""
        t = _tile_list(tiles)
        _check(lib().pt_render_tile_list(self._h, C.byref(cam), C.byref(prm), _ptr(t), t.size, C.c_void_p(d_tiles_ptr),
                                         C.c_void_p(d_work_ptr), C.c_void_p(stream_ptr)), "pt_render_tile_list")

    def render_tile_list(self, cam, prm, tiles):
        """The listed tiles, synchronous: (n, 8, 8, 3) float32, [i, ty, tx] = pixel (tx, ty) of tile tiles[i]; pixels outside
        the frame are 0.  torch provides the device buffers."""
        import torch
        t = _tile_list(tiles)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            out = torch.empty(tile_list_floats(t.size), dtype=torch.float32, device=dev)
            work = torch.empty(tile_list_work_bytes(cam, prm, t.size), dtype=torch.uint8, device=dev)
            self.render_tile_list_device(cam, prm, t, out.data_ptr(), work.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            return out.cpu().numpy().reshape(t.size, TILE, TILE, 3)

    def render_window(self, cam, prm, window):
        """The pixel window (x0, y0, x1, y1), half-open, synchronous: (y1 - y0, x1 - x0, 3) float32, bit for bit
        render(cam, prm)[y0:y1, x0:x1]; only the tiles that overlap the window are rendered."""
        x0, y0, x1, y1 = (int(v) for v in window)
        out = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0), 3), np.float32)
        _check(lib().pt_render_window(self._h, C.byref(cam), C.byref(prm), x0, y0, x1, y1, _ptr(out)), "pt_render_window")
        return out

    def render_views_device(self, cams, prm, d_tiles_ptr, d_work_ptr, stream_ptr=0, first_pass=None):
        """Device-resident render of a batch of cameras of one size in one pipeline run (raw device pointers: views_floats(cams[0],
        n) floats, view-major, and views_work_bytes(cams[0], prm, n) bytes), enqueued on the given stream; blocks until the render
        has drained.  first_pass: one first pass per view, or None for prm.first_pass (include/pt_api.h: pt_render_views)."""
        arr = _camera_array(cams)
        fp = _first_passes(first_pass, len(arr))
        _check(lib().pt_render_views(self._h, arr, len(arr), C.byref(prm), _ptr(fp) if fp is not None else None, C.c_void_p(d_tiles_ptr),
                                     C.c_void_p(d_work_ptr), C.c_void_p(stream_ptr)), "pt_render_views")

    def render_views(self, cams, prm, first_pass=None):
        """A batch of cameras of one size, synchronous: (V, H, W, 3) float32, [v] bit for bit render(cams[v], prm) (with
        first_pass[v] as its first pass where given)."""
        arr = _camera_array(cams)
        fp = _first_passes(first_pass, len(arr))
        out = np.zeros((len(arr), arr[0].H, arr[0].W, 3), np.float32)
        _check(lib().pt_render_views_host(self._h, arr, len(arr), C.byref(prm), _ptr(fp) if fp is not None else None, _ptr(out)),
               "pt_render_views_host")
        return out

    def update_vertices(self, pos, frames=None, stream_ptr=0):
        """Move the triangles (include/pt_api.h: pt_scene_update_vertices).  pos: n_tris x 9 (or n_tris x 3 x 3) float32, V0 V1 V2 in
        the order of the `tris` given at upload; frames: None (keep the shading frames) or n_tris x 27 float32, N0 N1 N2 T0 T1 T2
        B0 B1 B2.  torch tensors on the scene's device are used in place (data_ptr()), enqueued on stream_ptr, and must stay alive
        until the stream has passed the update; numpy arrays go through pt_scene_update_vertices_host (synchronous)."""
        n = self.n_tris
        if isinstance(pos, np.ndarray):
            if frames is not None and not isinstance(frames, np.ndarray):
                raise PtError("update_vertices: pos and frames must both be numpy arrays or both be torch tensors")
            p = np.ascontiguousarray(pos, np.float32)
            if p.size != n * 9 or p.shape[0] != n:
                raise PtError(f"update_vertices: pos has shape {p.shape}, the scene has {n} triangles")
            f = None
            if frames is not None:
                f = np.ascontiguousarray(frames, np.float32)
                if f.size != n * 27 or f.shape[0] != n:
                    raise PtError(f"update_vertices: frames has shape {f.shape}, want ({n}, 27)")
            _check(lib().pt_scene_update_vertices_host(self._h, _ptr(p), _ptr(f) if f is not None else None), "pt_scene_update_vertices_host")
            return
        for name, t, per in (("pos", pos, 9), ("frames", frames, 27)):
            if t is None:
                continue
            if not (hasattr(t, "data_ptr") and hasattr(t, "is_contiguous")):
                raise PtError(f"update_vertices: {name} must be a torch tensor or a numpy array")
            if str(t.dtype) != "torch.float32" or not t.is_contiguous() or t.numel() != n * per or t.shape[0] != n:
                raise PtError(f"update_vertices: {name} must be contiguous float32 with {n} x {per} elements, got {t.dtype} {tuple(t.shape)}")
            if t.device.type != "cuda" or t.device.index != self.device:
                raise PtError(f"update_vertices: {name} is on {t.device}, the scene is on device {self.device}")
        _check(lib().pt_scene_update_vertices(self._h, C.c_void_p(pos.data_ptr()), C.c_void_p(frames.data_ptr()) if frames is not None else None,
                                              C.c_void_p(stream_ptr)), "pt_scene_update_vertices")

    def update_spheres(self, spheres):
        """Move the analytic spheres: (n, 16) float32 records of the uploaded count; centre and radius may change, materials may not."""
        sph = np.ascontiguousarray(spheres, np.float32).reshape(-1, SPHERE_FLOATS)
        _check(lib().pt_scene_update_spheres(self._h, _ptr(sph), sph.shape[0]), "pt_scene_update_spheres")

    def update_materials(self, mat, stream_ptr=0):
        """Give every triangle a new material (include/pt_api.h: pt_scene_update_materials).  mat: (n_tris, 12) float32, emittance
        albedo specular opacity roughness metallic in the order of the `tris` given at upload; the set of lights follows the new
        emittances.  A torch tensor on the scene's device is used in place (data_ptr()), enqueued on stream_ptr; the call waits for
        that stream once, and the tensor is free when it returns.  A numpy array goes through pt_scene_update_materials_host."""
        n = self.n_tris
        if isinstance(mat, np.ndarray):
            m = np.ascontiguousarray(mat, np.float32)
            if m.size != n * 12 or m.shape[0] != n:
                raise PtError(f"update_materials: mat has shape {m.shape}, the scene has {n} triangles")
            _check(lib().pt_scene_update_materials_host(self._h, _ptr(m)), "pt_scene_update_materials_host")
            return
        if not (hasattr(mat, "data_ptr") and hasattr(mat, "is_contiguous")):
            raise PtError("update_materials: mat must be a torch tensor or a numpy array")
        if str(mat.dtype) != "torch.float32" or not mat.is_contiguous() or mat.numel() != n * 12 or mat.shape[0] != n:
            raise PtError(f"update_materials: mat must be contiguous float32 with {n} x 12 elements, got {mat.dtype} {tuple(mat.shape)}")
        if mat.device.type != "cuda" or mat.device.index != self.device:
            raise PtError(f"update_materials: mat is on {mat.device}, the scene is on device {self.device}")
        _check(lib().pt_scene_update_materials(self._h, C.c_void_p(mat.data_ptr()), C.c_void_p(stream_ptr)), "pt_scene_update_materials")

    def update_sphere_materials(self, spheres):
        """New records for the analytic spheres: (n, 16) float32 of the uploaded count; centre, radius and material may all change."""
        sph = np.ascontiguousarray(spheres, np.float32).reshape(-1, SPHERE_FLOATS)
        _check(lib().pt_scene_update_sphere_materials(self._h, _ptr(sph), sph.shape[0]), "pt_scene_update_sphere_materials")

    @property
    def nee_prune(self):
        """DevScene::nee_prune as the next render will see it (parity hook)."""
        return lib().pt_scene_nee_prune(self._h)

    def tree_inflation(self):
        """Summed box area of the binary traversal tree now / at upload (1.0 for a scene never updated); waits for the device."""
        r = C.c_double(0.0)
        _check(lib().pt_scene_tree_inflation(self._h, C.byref(r)), "pt_scene_tree_inflation")
        return r.value

    def rebuild_tree(self, stream_ptr=0, depth_budget=None, large_fraction=None):
        """Build both traversal trees anew on the GPU from the scene's current positions (include/pt_api.h: pt_scene_rebuild_tree),
        enqueued on stream_ptr; the call waits for that stream.  Every result stays bit for bit what it was.
        With a depth_budget or a large_fraction the call is pt_scene_rebuild_tree_ex (a None among the two takes its default,
        pt_rebuild_params_default) and returns its report as a dict: n_large, n_flattened_tris."""
        if depth_budget is None and large_fraction is None:
            return _check(lib().pt_scene_rebuild_tree(self._h, C.c_void_p(stream_ptr)), "pt_scene_rebuild_tree")
        prm, report = _rebuild_params(depth_budget, large_fraction), PtRebuildReport()
        _check(lib().pt_scene_rebuild_tree_ex(self._h, C.byref(prm), C.byref(report), C.c_void_p(stream_ptr)), "pt_scene_rebuild_tree_ex")
        return {name: int(getattr(report, name)) for name, _ in PtRebuildReport._fields_}

    def rebuild_tree_optimized(self, passes=None, depth_budget=None, large_fraction=None, stream_ptr=0):
        """rebuild_tree with a depth budget and size classes, then `passes` treelet restructuring passes by surface area
        (include/pt_api.h: pt_scene_rebuild_tree_opt).  A None takes its default (pt_rebuild_opt_passes_default,
        pt_rebuild_params_default).  Returns the report as a dict: n_large, n_flattened_tris, n_roots, n_restructured."""
        prm, report = _rebuild_params(depth_budget, large_fraction), PtRebuildOptReport()
        if passes is None:
            passes = lib().pt_rebuild_opt_passes_default()
        _check(lib().pt_scene_rebuild_tree_opt(self._h, C.byref(prm), passes, C.byref(report), C.c_void_p(stream_ptr)), "pt_scene_rebuild_tree_opt")
        return {name: int(getattr(report, name)) for name, _ in PtRebuildOptReport._fields_}

    def tree_info(self):
        """The traversal trees as they are now, from upload or from the last rebuild_tree: a dict with n_wide, n_quad, depth,
        quad_depth and the number of rebuilds so far.  No device call."""
        info = PtTreeInfo()
        _check(lib().pt_scene_tree_info(self._h, C.byref(info)), "pt_scene_tree_info")
        return {name: int(getattr(info, name)) for name, _ in PtTreeInfo._fields_}

    def _filtered(self, who, a, rays, filter, run, unfiltered, boxes=False, rows=None):
        """A query method's path with filter=: `a` (rays if `rays`, BOX8 records if `boxes`, else points; numpy is moved to the scene's device with torch, a torch
        tensor is used in place) and the filter's struct go to run(tensor, n, byref(struct)), the device path over the _f entry point,
        which returns torch tensors; numpy input gets numpy arrays back, after a wait.  An empty numpy input has nothing to filter and
        no device address: after the filter's checks it takes unfiltered(), the method's own numpy path, which returns the empty arrays.
        rows = (name, width): `a` is rows of `width` floats that the caller has checked already (the convex regions' planes)."""
        if not isinstance(filter, QueryFilter):
            raise PtError(f"{who}: filter must be a ptamd.QueryFilter")
        host = isinstance(a, np.ndarray)
        if host:
            x, n = _host_rows(who, a, *rows) if rows else _host_rows(who, a, "boxes" if boxes else "rays" if rays else "points", 8 if rays or boxes else 4)
        elif rows:
            n = a.shape[0]
        else:
            n = (_device_boxes if boxes else _device_rays if rays else _device_points)(who, a, self.device)
        if host and n == 0:
            filter._checks(who, self.device, n, self.n_tris + self.n_spheres, rays)
            return unfiltered()
        fs = filter._bind(who, self.device, n, self.n_tris + self.n_spheres, rays)
        import torch
        if host:
            a = torch.from_numpy(x).to(f"cuda:{self.device}")
            torch.cuda.synchronize(self.device)      # the uploads, whatever stream the query goes to
        out = run(a, n, C.byref(fs))
        if not host:
            return out
        torch.cuda.synchronize(self.device)
        return tuple(np.ascontiguousarray(o.cpu().numpy()) for o in out) if isinstance(out, tuple) else out.cpu().numpy()

    def trace_rays(self, rays, any_hit=False, surface=False, stream_ptr=0, filter=None):
        """Cast the caller's rays (include/pt_api.h: pt_trace_rays).  rays: (n, 8) float32 RAY8 records, org.xyz dir.xyz 0 tmax.
        Returns (t, prim) — float32 and int32 of length n, a miss is (0, -1) — and, with surface=True (closest hit only), the (n, 29)
        HIT records of raycast() as a third item.  any_hit=True: prim >= 0 iff the closest-hit query hits; which hit is unspecified.
        A torch float32 tensor on the scene's device is used in place (data_ptr()): the query is enqueued on stream_ptr, the results
        are torch tensors on that device, valid once the stream has passed the query, and `rays` must stay alive until then.
        A numpy array goes through pt_trace_rays_host (synchronous) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        if any_hit and surface:
            raise PtError("trace_rays: an any-hit query has no surface record")
        mode = QUERY_ANY if any_hit else QUERY_CLOSEST
        if filter is not None:
            def run(d, n, f):
                import torch
                hits = torch.empty((n, 2), dtype=torch.int32, device=d.device)
                surf = torch.empty((n, 29), dtype=torch.float32, device=d.device) if surface else None
                _check(lib().pt_trace_rays_f(self._h, C.c_void_p(d.data_ptr()), n, mode, f, C.c_void_p(hits.data_ptr()),
                                             C.c_void_p(surf.data_ptr()) if surface else None, C.c_void_p(stream_ptr)), "pt_trace_rays_f")
                return _records(hits, surf)
            return self._filtered("trace_rays", rays, True, filter, run, lambda: self.trace_rays(rays, any_hit, surface, stream_ptr))
        if isinstance(rays, np.ndarray):
            r, n = _host_rows("trace_rays", rays, "rays", 8)
            hits, surf = _host_out((n,), HIT_DTYPE, surface, 29)
            _check(lib().pt_trace_rays_host(self._h, _ptr(r), n, mode, _ptr(hits), _ptr(surf) if surface else None), "pt_trace_rays_host")
            return _records(hits, surf)
        n = _device_rays("trace_rays", rays, self.device)
        import torch
        hits = torch.empty((n, 2), dtype=torch.int32, device=rays.device)      # PtRayHit: t's bits | prim
        surf = torch.empty((n, 29), dtype=torch.float32, device=rays.device) if surface else None
        _check(lib().pt_trace_rays(self._h, C.c_void_p(rays.data_ptr()), n, mode, C.c_void_p(hits.data_ptr()),
                                   C.c_void_p(surf.data_ptr()) if surface else None, C.c_void_p(stream_ptr)), "pt_trace_rays")
        return _records(hits, surf)

    def closest_points(self, points, any_within=False, detail=False, stream_ptr=0, filter=None):
        """The primitive nearest to each of the caller's points (include/pt_api.h: pt_closest_points).  points: (n, 4) float32 POINT4
        records, p.xyz radius (>= 0, inf allowed).  Returns (dist2, prim) — float32 and int32 of length n, a miss is (0, -1) — and, with
        detail=True (closest only), the (n, 8) detail records c.xyz v w side feature 0 as a third item.  any_within=True: prim >= 0 iff
        the closest query finds something within the radius; which primitive is unspecified.
        A torch float32 tensor on the scene's device is used in place (data_ptr()): the query is enqueued on stream_ptr, the results
        are torch tensors on that device, valid once the stream has passed the query, and `points` must stay alive until then.
        A numpy array goes through pt_closest_points_host (synchronous) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        if any_within and detail:
            raise PtError("closest_points: an any-within query has no detail record")
        mode = NEAREST_ANY if any_within else NEAREST_CLOSEST
        if filter is not None:
            def run(d, n, f):
                import torch
                res = torch.empty((n, 2), dtype=torch.int32, device=d.device)
                det = torch.empty((n, 8), dtype=torch.float32, device=d.device) if detail else None
                _check(lib().pt_closest_points_f(self._h, C.c_void_p(d.data_ptr()), n, mode, f, C.c_void_p(res.data_ptr()),
                                                 C.c_void_p(det.data_ptr()) if detail else None, C.c_void_p(stream_ptr)), "pt_closest_points_f")
                return _records(res, det)
            return self._filtered("closest_points", points, False, filter, run, lambda: self.closest_points(points, any_within, detail, stream_ptr))
        if isinstance(points, np.ndarray):
            p, n = _host_rows("closest_points", points, "points", 4)
            res, det = _host_out((n,), NEAREST_DTYPE, detail, 8)
            _check(lib().pt_closest_points_host(self._h, _ptr(p), n, mode, _ptr(res), _ptr(det) if detail else None), "pt_closest_points_host")
            return _records(res, det)
        n = _device_points("closest_points", points, self.device)
        import torch
        res = torch.empty((n, 2), dtype=torch.int32, device=points.device)      # PtNearest: dist2's bits | prim
        det = torch.empty((n, 8), dtype=torch.float32, device=points.device) if detail else None
        _check(lib().pt_closest_points(self._h, C.c_void_p(points.data_ptr()), n, mode, C.c_void_p(res.data_ptr()),
                                       C.c_void_p(det.data_ptr()) if detail else None, C.c_void_p(stream_ptr)), "pt_closest_points")
        return _records(res, det)

    def nearest_k(self, points, k, detail=False, stream_ptr=0, filter=None):
        """The k nearest primitives within each point's radius, sorted (include/pt_api.h: pt_nearest_k).  points: (n, 4) float32 POINT4
        records, p.xyz radius (>= 0, inf allowed); 1 <= k <= NEAREST_KMAX.  Returns (dist2, prim) — float32 and int32 of shape (n, k),
        nearest first, among equal dist2 the larger prim first, the slots past the last candidate (0, -1) — and, with detail=True, the
        (n, k, 8) detail records c.xyz v w side feature 0 as a third item (zeros in a miss slot).
        A torch float32 tensor on the scene's device is used in place (data_ptr()): the query is enqueued on stream_ptr, the results
        are torch tensors on that device, valid once the stream has passed the query, and `points` must stay alive until then.
        A numpy array goes through pt_nearest_k_host (synchronous) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        k = int(k)
        if not 1 <= k <= NEAREST_KMAX:
            raise PtError(f"nearest_k: k = {k}, want 1 .. {NEAREST_KMAX}")
        if filter is not None:
            def run(d, n, f):
                import torch
                res = torch.empty((n, k, 2), dtype=torch.int32, device=d.device)
                det = torch.empty((n, k, 8), dtype=torch.float32, device=d.device) if detail else None
                _check(lib().pt_nearest_k_f(self._h, C.c_void_p(d.data_ptr()), n, k, f, C.c_void_p(res.data_ptr()),
                                            C.c_void_p(det.data_ptr()) if detail else None, C.c_void_p(stream_ptr)), "pt_nearest_k_f")
                return _records(res, det)
            return self._filtered("nearest_k", points, False, filter, run, lambda: self.nearest_k(points, k, detail, stream_ptr))
        if isinstance(points, np.ndarray):
            p, n = _host_rows("nearest_k", points, "points", 4)
            res, det = _host_out((n, k), NEAREST_DTYPE, detail, 8)
            _check(lib().pt_nearest_k_host(self._h, _ptr(p), n, k, _ptr(res), _ptr(det) if detail else None), "pt_nearest_k_host")
            return _records(res, det)
        n = _device_points("nearest_k", points, self.device)
        import torch
        res = torch.empty((n, k, 2), dtype=torch.int32, device=points.device)      # PtNearest: dist2's bits | prim
        det = torch.empty((n, k, 8), dtype=torch.float32, device=points.device) if detail else None
        _check(lib().pt_nearest_k(self._h, C.c_void_p(points.data_ptr()), n, k, C.c_void_p(res.data_ptr()),
                                  C.c_void_p(det.data_ptr()) if detail else None, C.c_void_p(stream_ptr)), "pt_nearest_k")
        return _records(res, det)

    def count_within(self, points, stream_ptr=0, filter=None):
        """How many primitives lie within each point's radius (include/pt_api.h: pt_count_within), uncapped: (n,) int32.  points as in
        nearest_k; an infinite radius counts every primitive, by walking the whole tree.  A torch tensor on the scene's device is
        used in place and the count is a torch tensor there, in stream order; a numpy array goes through pt_count_within_host.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        if filter is not None:
            def run(d, n, f):
                import torch
                cnt = torch.empty(n, dtype=torch.int32, device=d.device)
                _check(lib().pt_count_within_f(self._h, C.c_void_p(d.data_ptr()), n, f, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)),
                       "pt_count_within_f")
                return cnt
            return self._filtered("count_within", points, False, filter, run, lambda: self.count_within(points, stream_ptr))
        if isinstance(points, np.ndarray):
            p, n = _host_rows("count_within", points, "points", 4)
            cnt = np.zeros(n, np.int32)
            _check(lib().pt_count_within_host(self._h, _ptr(p), n, _ptr(cnt)), "pt_count_within_host")
            return cnt
        n = _device_points("count_within", points, self.device)
        import torch
        cnt = torch.empty(n, dtype=torch.int32, device=points.device)
        _check(lib().pt_count_within(self._h, C.c_void_p(points.data_ptr()), n, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_count_within")
        return cnt

    def trace_rays_k(self, rays, k, both_sides=False, detail=False, stream_ptr=0, filter=None):
        """The first k hits along each ray, sorted (include/pt_api.h: pt_trace_rays_k).  rays: (n, 8) float32 RAY8 records, org.xyz
        dir.xyz 0 tmax, as trace_rays takes them; 1 <= k <= RAY_HITS_KMAX.  Returns (t, prim) — float32 and int32 of shape (n, k), nearest
        first, among equal t the larger prim first, the slots past the last hit (0, -1) — and, with detail=True, the (n, k, 4) detail
        records u/det v/det facing 0 as a third item (zeros in a miss slot).  both_sides=True: back faces and the far root of a sphere
        count too (HITS_BOTH_SIDES); with False column 0 is trace_rays' closest hit.
        A torch float32 tensor on the scene's device is used in place (data_ptr()): the query is enqueued on stream_ptr, the results
        are torch tensors on that device, valid once the stream has passed the query, and `rays` must stay alive until then.
        A numpy array goes through pt_trace_rays_k_host (synchronous) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        k = int(k)
        if not 1 <= k <= RAY_HITS_KMAX:
            raise PtError(f"trace_rays_k: k = {k}, want 1 .. {RAY_HITS_KMAX}")
        flags = HITS_BOTH_SIDES if both_sides else HITS_FRONT
        if filter is not None:
            def run(d, n, f):
                import torch
                hits = torch.empty((n, k, 2), dtype=torch.int32, device=d.device)
                det = torch.empty((n, k, 4), dtype=torch.float32, device=d.device) if detail else None
                _check(lib().pt_trace_rays_k_f(self._h, C.c_void_p(d.data_ptr()), n, k, flags, f, C.c_void_p(hits.data_ptr()),
                                               C.c_void_p(det.data_ptr()) if detail else None, C.c_void_p(stream_ptr)), "pt_trace_rays_k_f")
                return _records(hits, det)
            return self._filtered("trace_rays_k", rays, True, filter, run, lambda: self.trace_rays_k(rays, k, both_sides, detail, stream_ptr))
        if isinstance(rays, np.ndarray):
            r, n = _host_rows("trace_rays_k", rays, "rays", 8)
            hits, det = _host_out((n, k), HIT_DTYPE, detail, 4)
            _check(lib().pt_trace_rays_k_host(self._h, _ptr(r), n, k, flags, _ptr(hits), _ptr(det) if detail else None), "pt_trace_rays_k_host")
            return _records(hits, det)
        n = _device_rays("trace_rays_k", rays, self.device)
        import torch
        hits = torch.empty((n, k, 2), dtype=torch.int32, device=rays.device)      # PtRayHit: t's bits | prim
        det = torch.empty((n, k, 4), dtype=torch.float32, device=rays.device) if detail else None
        _check(lib().pt_trace_rays_k(self._h, C.c_void_p(rays.data_ptr()), n, k, flags, C.c_void_p(hits.data_ptr()),
                                     C.c_void_p(det.data_ptr()) if detail else None, C.c_void_p(stream_ptr)), "pt_trace_rays_k")
        return _records(hits, det)

    def count_hits(self, rays, both_sides=False, stream_ptr=0, filter=None):
        """How many hits each ray has in [0, tmax] (include/pt_api.h: pt_count_hits), uncapped: (n,) int32.  rays and both_sides as in
        trace_rays_k.  A torch tensor on the scene's device is used in place and the count is a torch tensor there, in stream order; a
        numpy array goes through pt_count_hits_host.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        flags = HITS_BOTH_SIDES if both_sides else HITS_FRONT
        if filter is not None:
            def run(d, n, f):
                import torch
                cnt = torch.empty(n, dtype=torch.int32, device=d.device)
                _check(lib().pt_count_hits_f(self._h, C.c_void_p(d.data_ptr()), n, flags, f, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)),
                       "pt_count_hits_f")
                return cnt
            return self._filtered("count_hits", rays, True, filter, run, lambda: self.count_hits(rays, both_sides, stream_ptr))
        if isinstance(rays, np.ndarray):
            r, n = _host_rows("count_hits", rays, "rays", 8)
            cnt = np.zeros(n, np.int32)
            _check(lib().pt_count_hits_host(self._h, _ptr(r), n, flags, _ptr(cnt)), "pt_count_hits_host")
            return cnt
        n = _device_rays("count_hits", rays, self.device)
        import torch
        cnt = torch.empty(n, dtype=torch.int32, device=rays.device)
        _check(lib().pt_count_hits(self._h, C.c_void_p(rays.data_ptr()), n, flags, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_count_hits")
        return cnt

    def trace_rays_all(self, rays, both_sides=False, detail=False, stream_ptr=0, filter=None):
        """Every hit along each ray, sorted, in CSR form (include/pt_api.h: pt_trace_rays_list).  rays and both_sides as in trace_rays_k.
        Returns (offsets, t, prim) — int64 of shape (n + 1,), the hits of ray i at [offsets[i], offsets[i + 1]) of the float32 and int32
        arrays t and prim, nearest first, among equal t the larger prim first — and, with detail=True, the (total, 4) detail records
        u/det v/det facing 0 as a fourth item.
        A torch float32 tensor on the scene's device runs in place on stream_ptr: count_hits, list_offsets, one 8-byte read-back of the
        total — which WAITS for the stream to pass the scan —, the allocation of the records, the fill.  The records are torch tensors on
        that device, valid once the stream has passed the fill, and `rays` must stay alive until then.  A numpy array goes through
        pt_trace_rays_list_host (synchronous: a sizing call, then the fill) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        flags = HITS_BOTH_SIDES if both_sides else HITS_FRONT
        if filter is not None:
            def run(d, n, f):
                return _csr("trace_rays_all", d, "rays", 8, HIT_DTYPE, 4, detail, stream_ptr, self.device, _device_rays,
                            lambda t: self.count_hits(t, both_sides=both_sides, stream_ptr=stream_ptr, filter=filter), None,
                            lambda r, n, off, cap, out, det: _check(lib().pt_trace_rays_list_f(self._h, r, n, flags, off, cap, f, out, det,
                                                                                               C.c_void_p(stream_ptr)), "pt_trace_rays_list_f"))
            return self._filtered("trace_rays_all", rays, True, filter, run, lambda: self.trace_rays_all(rays, both_sides, detail, stream_ptr))
        return _csr("trace_rays_all", rays, "rays", 8, HIT_DTYPE, 4, detail, stream_ptr, self.device, _device_rays,
                         lambda d: self.count_hits(d, both_sides=both_sides, stream_ptr=stream_ptr),
                         lambda r, n, off, cap, out, det: _check(lib().pt_trace_rays_list_host(self._h, r, n, flags, off, cap, out, det),
                                                                 "pt_trace_rays_list_host"),
                         lambda r, n, off, cap, out, det: _check(lib().pt_trace_rays_list(self._h, r, n, flags, off, cap, out, det,
                                                                                          C.c_void_p(stream_ptr)), "pt_trace_rays_list"))

    def within_radius(self, points, detail=False, stream_ptr=0, filter=None):
        """Every primitive within each point's radius, sorted, in CSR form (include/pt_api.h: pt_within_radius_list).  points as in
        nearest_k; an infinite radius lists every primitive.  Returns (offsets, dist2, prim) — int64 of shape (n + 1,), the members of
        point i at [offsets[i], offsets[i + 1]) of the float32 and int32 arrays dist2 and prim, nearest first, among equal dist2 the larger
        prim first — and, with detail=True, the (total, 8) detail records c.xyz v w side feature 0 as a fourth item.
        A torch float32 tensor on the scene's device runs in place on stream_ptr: count_within, list_offsets, one 8-byte read-back of the
        total — which WAITS for the stream to pass the scan —, the allocation of the records, the fill.  The records are torch tensors on
        that device, valid once the stream has passed the fill, and `points` must stay alive until then.  A numpy array goes through
        pt_within_radius_list_host (synchronous: a sizing call, then the fill) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        if filter is not None:
            def run(d, n, f):
                return _csr("within_radius", d, "points", 4, NEAREST_DTYPE, 8, detail, stream_ptr, self.device, _device_points,
                            lambda t: self.count_within(t, stream_ptr=stream_ptr, filter=filter), None,
                            lambda p, n, off, cap, out, det: _check(lib().pt_within_radius_list_f(self._h, p, n, off, cap, f, out, det,
                                                                                                  C.c_void_p(stream_ptr)), "pt_within_radius_list_f"))
            return self._filtered("within_radius", points, False, filter, run, lambda: self.within_radius(points, detail, stream_ptr))
        return _csr("within_radius", points, "points", 4, NEAREST_DTYPE, 8, detail, stream_ptr, self.device, _device_points,
                         lambda d: self.count_within(d, stream_ptr=stream_ptr),
                         lambda p, n, off, cap, out, det: _check(lib().pt_within_radius_list_host(self._h, p, n, off, cap, out, det),
                                                                 "pt_within_radius_list_host"),
                         lambda p, n, off, cap, out, det: _check(lib().pt_within_radius_list(self._h, p, n, off, cap, out, det,
                                                                                             C.c_void_p(stream_ptr)), "pt_within_radius_list"))

    def box_count(self, boxes, inside=False, stream_ptr=0, filter=None):
        """How many primitives lie inside or touch each of the caller's axis-aligned boxes (include/pt_api.h: pt_box_count): (n,) int32.
        boxes: (n, 8) float32 BOX8 records, lo.xyz 0 hi.xyz 0 (grid_boxes makes those of a regular grid).  inside=True: only the
        primitives wholly inside.  An inverted box or one with a NaN holds nothing.  A torch tensor on the scene's device is used in
        place and the count is a torch tensor there, in stream order; a numpy array goes through pt_box_count_host.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        flags = BOX_INSIDE if inside else BOX_TOUCHING
        if filter is not None:
            def run(d, n, f):
                import torch
                cnt = torch.empty(n, dtype=torch.int32, device=d.device)
                _check(lib().pt_box_count(self._h, C.c_void_p(d.data_ptr()), n, flags, f, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_box_count")
                return cnt
            return self._filtered("box_count", boxes, False, filter, run, lambda: self.box_count(boxes, inside, stream_ptr), boxes=True)
        if isinstance(boxes, np.ndarray):
            b, n = _host_rows("box_count", boxes, "boxes", 8)
            cnt = np.zeros(n, np.int32)
            _check(lib().pt_box_count_host(self._h, _ptr(b), n, flags, _ptr(cnt)), "pt_box_count_host")
            return cnt
        n = _device_boxes("box_count", boxes, self.device)
        import torch
        cnt = torch.empty(n, dtype=torch.int32, device=boxes.device)
        _check(lib().pt_box_count(self._h, C.c_void_p(boxes.data_ptr()), n, flags, None, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_box_count")
        return cnt

    def box_any(self, boxes, inside=False, stream_ptr=0, filter=None):
        """Does anything lie inside or touch each box (include/pt_api.h: pt_box_any)?  Returns (cls, prim) — float32 and int32 of length
        n: prim >= 0 exactly when box_count of the same box is above 0, and then some member with its class, 0 = inside, 1 = touching
        (which member is unspecified); else the miss (0, -1).  boxes, inside, stream_ptr and filter as in box_count."""
        flags = BOX_INSIDE if inside else BOX_TOUCHING
        if filter is not None:
            def run(d, n, f):
                import torch
                res = torch.empty((n, 2), dtype=torch.int32, device=d.device)
                _check(lib().pt_box_any(self._h, C.c_void_p(d.data_ptr()), n, flags, f, C.c_void_p(res.data_ptr()), C.c_void_p(stream_ptr)), "pt_box_any")
                return _records(res, None)
            return self._filtered("box_any", boxes, False, filter, run, lambda: self.box_any(boxes, inside, stream_ptr), boxes=True)
        if isinstance(boxes, np.ndarray):
            b, n = _host_rows("box_any", boxes, "boxes", 8)
            res = np.zeros(n, BOX_DTYPE)
            _check(lib().pt_box_any_host(self._h, _ptr(b), n, flags, _ptr(res)), "pt_box_any_host")
            return _records(res, None)
        n = _device_boxes("box_any", boxes, self.device)
        import torch
        res = torch.empty((n, 2), dtype=torch.int32, device=boxes.device)      # PtBoxMember: cls's bits | prim
        _check(lib().pt_box_any(self._h, C.c_void_p(boxes.data_ptr()), n, flags, None, C.c_void_p(res.data_ptr()), C.c_void_p(stream_ptr)), "pt_box_any")
        return _records(res, None)

    def in_boxes(self, boxes, inside=False, stream_ptr=0, filter=None):
        """Every primitive inside or touching each box, in CSR form (include/pt_api.h: pt_box_list).  Returns (offsets, cls, prim) — int64
        of shape (n + 1,), the members of box i at [offsets[i], offsets[i + 1]) of the float32 and int32 arrays cls and prim: the
        primitives inside (cls 0) first, then the touching ones (cls 1), within a class the larger prim first.  boxes and inside as in
        box_count.  A torch float32 tensor on the scene's device runs in place on stream_ptr: box_count, list_offsets, one 8-byte
        read-back of the total — which WAITS for the stream to pass the scan —, the allocation of the records, the fill.  A numpy array
        goes through pt_box_list_host (synchronous: a sizing call, then the fill) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        flags = BOX_INSIDE if inside else BOX_TOUCHING
        if filter is not None:
            def run(d, n, f):
                return _csr("in_boxes", d, "boxes", 8, BOX_DTYPE, 0, False, stream_ptr, self.device, _device_boxes,
                            lambda t: self.box_count(t, inside, stream_ptr=stream_ptr, filter=filter), None,
                            lambda b, n, off, cap, out, det: _check(lib().pt_box_list(self._h, b, n, flags, off, cap, f, out, C.c_void_p(stream_ptr)),
                                                                    "pt_box_list"))
            return self._filtered("in_boxes", boxes, False, filter, run, lambda: self.in_boxes(boxes, inside, stream_ptr), boxes=True)
        return _csr("in_boxes", boxes, "boxes", 8, BOX_DTYPE, 0, False, stream_ptr, self.device, _device_boxes,
                    lambda d: self.box_count(d, inside, stream_ptr=stream_ptr),
                    lambda b, n, off, cap, out, det: _check(lib().pt_box_list_host(self._h, b, n, flags, off, cap, out), "pt_box_list_host"),
                    lambda b, n, off, cap, out, det: _check(lib().pt_box_list(self._h, b, n, flags, off, cap, None, out, C.c_void_p(stream_ptr)),
                                                            "pt_box_list"))

    def voxelize(self, lo, hi, shape, inside=False, filter=None):
        """The scene as an occupancy grid: the (nz, ny, nx) int32 counts of box_count over grid_boxes(lo, hi, shape) on the scene's
        device, a torch tensor there (NULL stream).  Neighbouring voxels share their faces bit for bit and touching counts, so a
        primitive that touches a shared face counts in BOTH voxels: the counts do not sum to the number of primitives.  inside and
        filter as in box_count."""
        boxes = grid_boxes(lo, hi, shape, device=self.device)
        nx, ny, nz = (int(v) for v in shape)
        return self.box_count(boxes, inside=inside, filter=filter).view(nz, ny, nx)

    def convex_count(self, planes, inside=False, stream_ptr=0, filter=None):
        """How many primitives lie inside or touch each of the caller's convex regions (include/pt_api.h: pt_convex_count): (n,) int32.
        planes: (n, m, 4) float32 PLANE4 records n.xyz | d, 1 <= m <= CONVEX_MAX_PLANES, region i the points x with n . x <= d for
        all m of its planes (frustum_planes, obb_planes and aabb_planes make them; pad a region of fewer planes with (0, 0, 0, 0)).
        inside=True: only the primitives wholly inside.  A region with a NaN or an infinite normal holds nothing.  A torch tensor on
        the scene's device is used in place and the count is a torch tensor there, in stream order; a numpy array goes through
        pt_convex_count_host.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        flags = CONVEX_INSIDE if inside else CONVEX_TOUCHING
        x, n, m = _convex_planes("convex_count", planes, self.device)
        if filter is not None:
            def run(d, n, f):
                import torch
                cnt = torch.empty(n, dtype=torch.int32, device=d.device)
                _check(lib().pt_convex_count(self._h, C.c_void_p(d.data_ptr()), n, m, flags, f, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_convex_count")
                return cnt
            return self._filtered("convex_count", x, False, filter, run, lambda: self.convex_count(planes, inside, stream_ptr), rows=("planes", 4 * m))
        if isinstance(x, np.ndarray):
            cnt = np.zeros(n, np.int32)
            _check(lib().pt_convex_count_host(self._h, _ptr(x), n, m, flags, _ptr(cnt)), "pt_convex_count_host")
            return cnt
        import torch
        cnt = torch.empty(n, dtype=torch.int32, device=x.device)
        _check(lib().pt_convex_count(self._h, C.c_void_p(x.data_ptr()), n, m, flags, None, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_convex_count")
        return cnt

    def convex_any(self, planes, inside=False, stream_ptr=0, filter=None):
        """Does anything lie inside or touch each region (include/pt_api.h: pt_convex_any)?  Returns (cls, prim) — float32 and int32 of
        length n: prim >= 0 exactly when convex_count of the same region is above 0, and then some member with its class, 0 = inside,
        1 = touching (which member is unspecified); else the miss (0, -1).  planes, inside, stream_ptr and filter as in convex_count."""
        flags = CONVEX_INSIDE if inside else CONVEX_TOUCHING
        x, n, m = _convex_planes("convex_any", planes, self.device)
        if filter is not None:
            def run(d, n, f):
                import torch
                res = torch.empty((n, 2), dtype=torch.int32, device=d.device)
                _check(lib().pt_convex_any(self._h, C.c_void_p(d.data_ptr()), n, m, flags, f, C.c_void_p(res.data_ptr()), C.c_void_p(stream_ptr)), "pt_convex_any")
                return _records(res, None)
            return self._filtered("convex_any", x, False, filter, run, lambda: self.convex_any(planes, inside, stream_ptr), rows=("planes", 4 * m))
        if isinstance(x, np.ndarray):
            res = np.zeros(n, BOX_DTYPE)
            _check(lib().pt_convex_any_host(self._h, _ptr(x), n, m, flags, _ptr(res)), "pt_convex_any_host")
            return _records(res, None)
        import torch
        res = torch.empty((n, 2), dtype=torch.int32, device=x.device)      # PtBoxMember: cls's bits | prim
        _check(lib().pt_convex_any(self._h, C.c_void_p(x.data_ptr()), n, m, flags, None, C.c_void_p(res.data_ptr()), C.c_void_p(stream_ptr)), "pt_convex_any")
        return _records(res, None)

    def in_convex(self, planes, inside=False, stream_ptr=0, filter=None):
        """Every primitive inside or touching each region, in CSR form (include/pt_api.h: pt_convex_list).  Returns (offsets, cls, prim)
        — int64 of shape (n + 1,), the members of region i at [offsets[i], offsets[i + 1]) of the float32 and int32 arrays cls and prim:
        the primitives inside (cls 0) first, then the touching ones (cls 1), within a class the larger prim first.  planes and inside as
        in convex_count.  A torch float32 tensor on the scene's device runs in place on stream_ptr: convex_count, list_offsets, one
        8-byte read-back of the total — which WAITS for the stream to pass the scan —, the allocation of the records, the fill.  A
        numpy array goes through pt_convex_list_host (synchronous: a sizing call, then the fill) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        flags = CONVEX_INSIDE if inside else CONVEX_TOUCHING
        x, n, m = _convex_planes("in_convex", planes, self.device)
        checked = lambda who, a, device: a.shape[0]      # noqa: E731  (the rows of x are checked)
        if filter is not None:
            def run(d, n, f):
                return _csr("in_convex", d, "planes", 4 * m, BOX_DTYPE, 0, False, stream_ptr, self.device, checked,
                            lambda t: self.convex_count(t.view(-1, m, 4), inside, stream_ptr=stream_ptr, filter=filter), None,
                            lambda b, n, off, cap, out, det: _check(lib().pt_convex_list(self._h, b, n, m, flags, off, cap, f, out, C.c_void_p(stream_ptr)),
                                                                    "pt_convex_list"))
            return self._filtered("in_convex", x, False, filter, run, lambda: self.in_convex(planes, inside, stream_ptr), rows=("planes", 4 * m))
        return _csr("in_convex", x, "planes", 4 * m, BOX_DTYPE, 0, False, stream_ptr, self.device, checked,
                    lambda d: self.convex_count(d.view(-1, m, 4), inside, stream_ptr=stream_ptr),
                    lambda b, n, off, cap, out, det: _check(lib().pt_convex_list_host(self._h, b, n, m, flags, off, cap, out), "pt_convex_list_host"),
                    lambda b, n, off, cap, out, det: _check(lib().pt_convex_list(self._h, b, n, m, flags, off, cap, None, out, C.c_void_p(stream_ptr)),
                                                            "pt_convex_list"))

    def select_window(self, cam, window, inside=False, filter=None):
        """The marquee selection: the indices, ascending (int32 numpy), of the primitives that touch (inside=True: lie wholly inside)
        the frustum of the pixel window (x0, y0, x1, y1) of `cam`, half-open and unbounded in depth (frustum_planes).  Touching is
        conservative near the frustum's edges, as convex_count states; filter as in convex_count."""
        _, _, prim = self.in_convex(frustum_planes(cam, window)[None], inside=inside, filter=filter)
        return np.sort(prim)

    def sweep_spheres(self, sweeps, any_hit=False, detail=False, stream_ptr=0, filter=None):
        """How far each of the caller's spheres travels before it touches the scene (include/pt_api.h: pt_sweep_spheres).  sweeps: (n, 8)
        float32 SWEEP8 records, org.xyz radius dir.xyz tmax (sweep_records makes them); the direction is not normalised, t is the
        parameter along it.  Returns (t, prim) — float32 and int32 of length n, a miss is (0, -1) — and, with detail=True (closest
        only), the (n, 8) detail records c.xyz v w side feature 0 of closest_points at the sphere's centre at contact as a third item.
        any_hit=True: prim >= 0 iff the closest form hits; which contact is unspecified.
        A torch float32 tensor on the scene's device is used in place (data_ptr()): the query is enqueued on stream_ptr, the results
        are torch tensors on that device, valid once the stream has passed the query, and `sweeps` must stay alive until then.
        A numpy array goes through pt_sweep_spheres_host (synchronous) and returns numpy arrays.
        filter: a QueryFilter without tmin (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        if any_hit and detail:
            raise PtError("sweep_spheres: an any-contact sweep has no detail record")
        mode = SWEEP_ANY if any_hit else SWEEP_CLOSEST

        def device_call(d, n, f):
            import torch
            hits = torch.empty((n, 2), dtype=torch.int32, device=d.device)      # PtRayHit: t's bits | prim
            det = torch.empty((n, 8), dtype=torch.float32, device=d.device) if detail else None
            _check(lib().pt_sweep_spheres(self._h, C.c_void_p(d.data_ptr()), n, mode, f, C.c_void_p(hits.data_ptr()),
                                          C.c_void_p(det.data_ptr()) if detail else None, C.c_void_p(stream_ptr)), "pt_sweep_spheres")
            return _records(hits, det)
        if filter is not None:
            if not isinstance(sweeps, np.ndarray):
                _device_sweeps("sweep_spheres", sweeps, self.device)
            return self._filtered("sweep_spheres", sweeps, False, filter, device_call, lambda: self.sweep_spheres(sweeps, any_hit, detail, stream_ptr),
                                  rows=("sweeps", 8))
        if isinstance(sweeps, np.ndarray):
            x, n = _host_rows("sweep_spheres", sweeps, "sweeps", 8)
            hits, det = _host_out((n,), HIT_DTYPE, detail, 8)
            _check(lib().pt_sweep_spheres_host(self._h, _ptr(x), n, mode, _ptr(hits), _ptr(det) if detail else None), "pt_sweep_spheres_host")
            return _records(hits, det)
        return device_call(sweeps, _device_sweeps("sweep_spheres", sweeps, self.device), None)

    def tri_count(self, tris, stream_ptr=0, filter=None, detail=False):
        """How many primitives each of the caller's triangles cuts (include/pt_api.h: pt_tri_count): (n,) int32.  tris: (n, 12) float32
        TRI12 records, a.xyz - b.xyz - c.xyz - (tri_records makes them).  A zero-area triangle or one with a NaN cuts no triangle.  A
        torch tensor on the scene's device is used in place and the count is a torch tensor there, in stream order; a numpy array
        goes through pt_tri_count_host.  Only cut_by_triangles returns segments: detail must stay False.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        if detail:
            raise PtError("tri_count: a detail buffer is allowed only on the list call (cut_by_triangles)")
        if filter is not None:
            def run(d, n, f):
                import torch
                cnt = torch.empty(n, dtype=torch.int32, device=d.device)
                _check(lib().pt_tri_count(self._h, C.c_void_p(d.data_ptr()), n, f, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_tri_count")
                return cnt
            if not isinstance(tris, np.ndarray):
                _device_tris("tri_count", tris, self.device)
            return self._filtered("tri_count", tris, False, filter, run, lambda: self.tri_count(tris, stream_ptr), rows=("tris", 12))
        if isinstance(tris, np.ndarray):
            x, n = _host_rows("tri_count", tris, "tris", 12)
            cnt = np.zeros(n, np.int32)
            _check(lib().pt_tri_count_host(self._h, _ptr(x), n, _ptr(cnt)), "pt_tri_count_host")
            return cnt
        n = _device_tris("tri_count", tris, self.device)
        import torch
        cnt = torch.empty(n, dtype=torch.int32, device=tris.device)
        _check(lib().pt_tri_count(self._h, C.c_void_p(tris.data_ptr()), n, None, C.c_void_p(cnt.data_ptr()), C.c_void_p(stream_ptr)), "pt_tri_count")
        return cnt

    def tri_any(self, tris, stream_ptr=0, filter=None, detail=False):
        """Does each triangle cut anything (include/pt_api.h: pt_tri_any)?  Returns (cls, prim) — float32 and int32 of length n: prim >= 0
        exactly when tri_count of the same record is above 0, and then some member with cls 1 (which member is unspecified); else the
        miss (0, -1).  tris, stream_ptr, filter and detail as in tri_count."""
        if detail:
            raise PtError("tri_any: a detail buffer is allowed only on the list call (cut_by_triangles)")
        if filter is not None:
            def run(d, n, f):
                import torch
                res = torch.empty((n, 2), dtype=torch.int32, device=d.device)
                _check(lib().pt_tri_any(self._h, C.c_void_p(d.data_ptr()), n, f, C.c_void_p(res.data_ptr()), C.c_void_p(stream_ptr)), "pt_tri_any")
                return _records(res, None)
            if not isinstance(tris, np.ndarray):
                _device_tris("tri_any", tris, self.device)
            return self._filtered("tri_any", tris, False, filter, run, lambda: self.tri_any(tris, stream_ptr), rows=("tris", 12))
        if isinstance(tris, np.ndarray):
            x, n = _host_rows("tri_any", tris, "tris", 12)
            res = np.zeros(n, BOX_DTYPE)
            _check(lib().pt_tri_any_host(self._h, _ptr(x), n, _ptr(res)), "pt_tri_any_host")
            return _records(res, None)
        n = _device_tris("tri_any", tris, self.device)
        import torch
        res = torch.empty((n, 2), dtype=torch.int32, device=tris.device)      # PtBoxMember: cls's bits | prim
        _check(lib().pt_tri_any(self._h, C.c_void_p(tris.data_ptr()), n, None, C.c_void_p(res.data_ptr()), C.c_void_p(stream_ptr)), "pt_tri_any")
        return _records(res, None)

    def cut_by_triangles(self, tris, segments=False, stream_ptr=0, filter=None):
        """Every primitive each triangle cuts, in CSR form (include/pt_api.h: pt_tri_list).  Returns (offsets, cls, prim) — int64 of shape
        (n + 1,), the members of triangle i at [offsets[i], offsets[i + 1]) of the float32 and int32 arrays cls (all 1) and prim, the
        larger prim first — and, with segments=True, the (total, 8) records p.xyz q.xyz kind 0 as a fourth item: the segment along
        which the two triangles cut (kind 1), or the query's point closest to a sphere's centre twice (kind 2).
        A torch float32 tensor on the scene's device runs in place on stream_ptr: tri_count, list_offsets, one 8-byte read-back of the
        total — which WAITS for the stream to pass the scan —, the allocation of the records, the fill.  A numpy array goes through
        pt_tri_list_host (synchronous: a sizing call, then the fill) and returns numpy arrays.
        filter: a QueryFilter (numpy input is then moved to the device with torch and comes back as numpy); None: no filter."""
        if filter is not None:
            def run(d, n, f):
                return _csr("cut_by_triangles", d, "tris", 12, BOX_DTYPE, 8, segments, stream_ptr, self.device, _device_tris,
                            lambda t: self.tri_count(t, stream_ptr=stream_ptr, filter=filter), None,
                            lambda b, n, off, cap, out, det: _check(lib().pt_tri_list(self._h, b, n, off, cap, f, out, det, C.c_void_p(stream_ptr)),
                                                                    "pt_tri_list"))
            if not isinstance(tris, np.ndarray):
                _device_tris("cut_by_triangles", tris, self.device)
            return self._filtered("cut_by_triangles", tris, False, filter, run, lambda: self.cut_by_triangles(tris, segments, stream_ptr),
                                  rows=("tris", 12))
        return _csr("cut_by_triangles", tris, "tris", 12, BOX_DTYPE, 8, segments, stream_ptr, self.device, _device_tris,
                    lambda d: self.tri_count(d, stream_ptr=stream_ptr),
                    lambda b, n, off, cap, out, det: _check(lib().pt_tri_list_host(self._h, b, n, off, cap, out, det), "pt_tri_list_host"),
                    lambda b, n, off, cap, out, det: _check(lib().pt_tri_list(self._h, b, n, off, cap, None, out, det, C.c_void_p(stream_ptr)),
                                                            "pt_tri_list"))

    def slice(self, point, normal, half_extent):
        """The plane section of the scene: the segments along which a square of the given half-extent, centred on `point` in the plane
        with that normal, cuts the scene's triangles (two query triangles that share the square's diagonal: quad_triangles).  Returns
        (segments, prim): (m, 2, 3) float32 end points and (m,) int32, the members of the first triangle and then of the second, each
        with the larger prim first; spheres are left out (their section is a circle, not a segment).  Synchronous, numpy."""
        quad = slice_triangles(point, normal, half_extent)      # its checks come before any device call
        _, _, prim, seg = self.cut_by_triangles(quad, segments=True)
        keep = seg[:, 6] == 1
        return np.ascontiguousarray(seg[keep, 0:6]).reshape(-1, 2, 3), np.ascontiguousarray(prim[keep])

    def render_rays_device(self, d_rays_ptr, n_rays, prm, d_rgb_ptr, d_work_ptr, d_seed_ptr=0, seed_stride=None, stream_ptr=0):
        """Device-resident radiance along n_rays RAY8 records (raw device pointers: rays_floats(n) floats of output, rays_work_bytes(prm,
        n) bytes of scratch, d_seed_ptr 0 = ray i is seeded with i), enqueued on the given stream; blocks until the render has drained.
        seed_stride defaults to n_rays (include/pt_api.h: pt_render_rays)."""
        n = int(n_rays)
        _check(lib().pt_render_rays(self._h, C.c_void_p(d_rays_ptr), C.c_void_p(d_seed_ptr or None), n, n if seed_stride is None else int(seed_stride),
                                    C.byref(prm), C.c_void_p(d_rgb_ptr), C.c_void_p(d_work_ptr), C.c_void_p(stream_ptr)), "pt_render_rays")

    def render_rays(self, rays, prm, seeds=None, seed_stride=None, stream_ptr=0):
        """Radiance along the caller's own rays (include/pt_api.h: pt_render_rays): ray i takes the place of a pixel.  rays: (n, 8)
        float32 RAY8 records, org.xyz dir.xyz 0 tmax, directions of unit length.  seeds: None (ray i is seeded with i) or n int32;
        pass k adds k * seed_stride, which defaults to n.  Returns (n, 3) float32, the sum over prm.passes passes of the per-pass means.
        A numpy array goes through pt_render_rays_host (synchronous) and returns a numpy array.  A torch float32 tensor on the scene's
        device is used in place (data_ptr(); seeds then a torch int32 tensor there, or None): the render runs on stream_ptr and the
        result is a torch tensor on that device, valid once the stream has passed the call."""
        if isinstance(rays, np.ndarray):
            r = np.ascontiguousarray(rays, np.float32)
            if r.ndim != 2 or r.shape[1] != 8:
                raise PtError(f"render_rays: rays has shape {r.shape}, want (n, 8)")
            n = r.shape[0]
            sd = None
            if seeds is not None:
                sd = np.ascontiguousarray(seeds, np.int32).reshape(-1)
                if sd.size != n:
                    raise PtError(f"render_rays: {sd.size} seeds for {n} rays")
            out = np.zeros((n, 3), np.float32)
            _check(lib().pt_render_rays_host(self._h, _ptr(r), _ptr(sd) if sd is not None else None, n, n if seed_stride is None else int(seed_stride),
                                             C.byref(prm), _ptr(out)), "pt_render_rays_host")
            return out
        if not (hasattr(rays, "data_ptr") and hasattr(rays, "is_contiguous")):
            raise PtError("render_rays: rays must be a torch tensor or a numpy array")
        if str(rays.dtype) != "torch.float32" or not rays.is_contiguous() or rays.dim() != 2 or rays.shape[1] != 8:
            raise PtError(f"render_rays: rays must be contiguous float32 of shape (n, 8), got {rays.dtype} {tuple(rays.shape)}")
        if rays.device.type != "cuda" or rays.device.index != self.device:
            raise PtError(f"render_rays: rays is on {rays.device}, the scene is on device {self.device}")
        n = rays.shape[0]
        if seeds is not None:
            if not hasattr(seeds, "data_ptr") or str(seeds.dtype) != "torch.int32" or not seeds.is_contiguous() or seeds.numel() != n or seeds.device != rays.device:
                raise PtError(f"render_rays: seeds must be a contiguous int32 tensor of {n} elements on {rays.device}")
        import torch
        with torch.cuda.device(rays.device):
            rgb = torch.empty(rays_floats(n), dtype=torch.float32, device=rays.device)
            work = torch.empty(rays_work_bytes(prm, n), dtype=torch.uint8, device=rays.device)
        self.render_rays_device(rays.data_ptr(), n, prm, rgb.data_ptr(), work.data_ptr(), seeds.data_ptr() if seeds is not None else 0, seed_stride, stream_ptr)
        return rgb[:3 * n].view(n, 3)

    def dbg_array(self, name):
        """pt_dbg_scene_array: one device array of the scene as a flat numpy array (SCENE_ARRAYS; layouts: csrc/pt_device.h)."""
        which, dt = SCENE_ARRAYS[name]
        size = lib().pt_dbg_scene_array(self._h, which, None, 0)
        if size < 0:
            _check(size, "pt_dbg_scene_array")
        out = np.zeros(size // 4, dt)
        if size and lib().pt_dbg_scene_array(self._h, which, _ptr(out), size) != size:
            raise PtError("pt_dbg_scene_array: " + lib().pt_last_error().decode())
        return out

    def raycast(self, rays8):
        rays8 = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        n = rays8.shape[0]
        hits = np.zeros((n, 29), np.float32)
        prim = np.zeros(n, np.int32)
        _check(lib().pt_dbg_raycast(self._h, _ptr(rays8), n, _ptr(hits), _ptr(prim)), "pt_dbg_raycast")
        return hits, prim


def _grid_edges(lo, hi, shape):
    """The per-axis edges of grid_boxes: three float32 arrays of n + 1 edges, lo + (hi - lo) * (i / n) in float32, the last one hi."""
    lo, hi = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        raise PtError(f"grid_boxes: lo and hi must be 3 finite floats each with lo <= hi, got {lo} {hi}")
    try:
        n = [int(v) for v in shape]
    except (TypeError, ValueError):
        raise PtError(f"grid_boxes: shape must be three ints (nx, ny, nz), got {shape!r}")
    if len(n) != 3 or min(n) < 1 or n[0] * n[1] * n[2] >= 1 << 31:
        raise PtError(f"grid_boxes: shape must be three ints >= 1 (nx, ny, nz) with fewer than 2^31 voxels, got {shape!r}")
    edges = []
    for a in range(3):
        e = (lo[a] + (hi[a] - lo[a]) * (np.arange(n[a] + 1, dtype=np.float32) / np.float32(n[a]))).astype(np.float32)
        e[n[a]] = hi[a]
        edges.append(e)
    return edges, n


def grid_boxes(lo, hi, shape, device=0):
    """The BOX8 records of the nx * ny * nz voxels of a regular grid over [lo, hi], x fastest (voxel (ix, iy, iz) is row
    (iz * ny + iy) * nx + ix): an (n, 8) float32 torch tensor on cuda:`device`; device=None: a numpy array.  Each axis's n + 1 edges are
    computed ONCE in float32, lo + (hi - lo) * (i / n), and the last is set to hi exactly: neighbouring voxels share a face bit for
    bit, so no primitive falls between two voxels, and one that touches a shared face is a member of both."""
    (ex, ey, ez), (nx, ny, nz) = _grid_edges(lo, hi, shape)
    b = np.zeros((nz, ny, nx, 8), np.float32)
    b[..., 0], b[..., 4] = ex[None, None, :-1], ex[None, None, 1:]
    b[..., 1], b[..., 5] = ey[None, :-1, None], ey[None, 1:, None]
    b[..., 2], b[..., 6] = ez[:-1, None, None], ez[1:, None, None]
    b = b.reshape(-1, 8)
    if device is None:
        return b
    import torch
    return torch.from_numpy(b).to(f"cuda:{int(device)}")


def _convex_planes(who, planes, device):
    """The host-side checks of a convex query's planes, (n, m, 4) float32 with 1 <= m <= CONVEX_MAX_PLANES, for the scene on `device`:
    a torch tensor there, or a numpy array.  Returns (the planes as n rows of 4 m floats, n, m)."""
    if isinstance(planes, np.ndarray):
        x = np.ascontiguousarray(planes, np.float32)
        shape = x.shape
    elif hasattr(planes, "data_ptr") and hasattr(planes, "is_contiguous"):
        x, shape = planes, tuple(planes.shape)
        if str(x.dtype) != "torch.float32" or not x.is_contiguous():
            raise PtError(f"{who}: planes must be contiguous float32 of shape (n, m, 4), got {x.dtype} {shape}")
    else:
        raise PtError(f"{who}: planes must be a torch tensor or a numpy array")
    if len(shape) != 3 or shape[2] != 4 or not 1 <= shape[1] <= CONVEX_MAX_PLANES:
        raise PtError(f"{who}: planes has shape {tuple(shape)}, want (n, m, 4) with 1 <= m <= {CONVEX_MAX_PLANES}")
    if not isinstance(x, np.ndarray) and (x.device.type != "cuda" or x.device.index != device):
        raise PtError(f"{who}: planes is on {x.device}, the scene is on device {device}")
    return x.reshape(shape[0], 4 * shape[1]), shape[0], shape[1]


def frustum_planes(cam, window=None, near=-1.0, far=float("inf")):
    """The six planes (left, right, top, bottom, near, far) of the frustum of a pixel window of `cam` (include/pt_api.h:
    pt_camera_frustum): (6, 4) float32 for Scene.convex_count and its kin.  window: (x0, y0, x1, y1), half-open, floats allowed, None:
    the whole frame; a list of windows gives (n, 6, 4).  near < 0: no near plane; far = inf: no far plane (the neutral plane
    (0, 0, 0, inf) stands in their place)."""
    if window is None:
        window = (0, 0, cam.W, cam.H)
    w = np.asarray(window, np.float32)
    if w.ndim not in (1, 2) or w.shape[-1] != 4:
        raise PtError(f"frustum_planes: window must be (x0, y0, x1, y1) or a list of such, got shape {w.shape}")
    out = np.zeros((len(w.reshape(-1, 4)), 6, 4), np.float32)
    for i, (x0, y0, x1, y1) in enumerate(w.reshape(-1, 4).tolist()):
        _check(lib().pt_camera_frustum(C.byref(cam), x0, y0, x1, y1, near, far, _ptr(out[i])), "pt_camera_frustum")
    return out[0] if w.ndim == 1 else out


def _planes64(normals, d):
    """(k, 4) float32 PLANE4 records from float64 normals and offsets, each rounded once"""
    return np.concatenate([normals, d[:, None]], 1).astype(np.float32)


def obb_planes(center, axes, half):
    """The six planes of an oriented box: (6, 4) float32, +axis_0, -axis_0, +axis_1, ...  axes: the three rows of a rotation; the planes
    are +-axis_k with d = +-axis_k . center + half_k, computed in float64 and rounded once."""
    c, a, h = np.asarray(center, np.float64).reshape(-1), np.asarray(axes, np.float64), np.asarray(half, np.float64).reshape(-1)
    if c.shape != (3,) or a.shape != (3, 3) or h.shape != (3,):
        raise PtError(f"obb_planes: want a center of 3, axes of (3, 3) and half sizes of 3, got {c.shape} {a.shape} {h.shape}")
    n = np.stack([a[0], -a[0], a[1], -a[1], a[2], -a[2]])
    return _planes64(n, n @ c + np.repeat(h, 2))


def sweep_records(org, dir, radius, tmax):
    """SWEEP8 records for Scene.sweep_spheres: (n, 8) float32, org.xyz | radius | dir.xyz | tmax.  org and dir: (n, 3) or 3 floats;
    radius and tmax: n floats or one.  The four broadcast against each other; a negative or NaN radius or tmax is refused."""
    o, d = np.asarray(org, np.float32), np.asarray(dir, np.float32)
    r, t = np.asarray(radius, np.float32), np.asarray(tmax, np.float32)
    if o.ndim not in (1, 2) or o.shape[-1] != 3 or d.ndim not in (1, 2) or d.shape[-1] != 3 or r.ndim > 1 or t.ndim > 1:
        raise PtError(f"sweep_records: want org and dir of shape (n, 3) or (3,), radius and tmax of n floats or one, got {o.shape} {d.shape} {r.shape} {t.shape}")
    if not ((r >= 0).all() and (t >= 0).all()):
        raise PtError("sweep_records: radius and tmax must be >= 0")
    try:
        n = np.broadcast_shapes(o.shape[:-1], d.shape[:-1], r.shape, t.shape)
    except ValueError:
        raise PtError(f"sweep_records: the lengths do not agree: {o.shape} {d.shape} {r.shape} {t.shape}") from None
    out = np.zeros(tuple(n or (1,)) + (8,), np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = o, r, d, t
    return out


def tri_records(a, b, c):
    """TRI12 records for Scene.tri_count, tri_any and cut_by_triangles: (n, 12) float32, a.xyz 0 b.xyz 0 c.xyz 0.  a, b, c: (n, 3) or 3
    floats each."""
    v = [np.atleast_2d(np.asarray(x, np.float32)) for x in (a, b, c)]
    if any(x.ndim != 2 or x.shape[1] != 3 for x in v):
        raise PtError(f"tri_records: want a, b and c of shape (n, 3) or (3,), got {[x.shape for x in v]}")
    try:
        v = np.broadcast_arrays(*v)
    except ValueError:
        raise PtError(f"tri_records: the lengths do not agree: {[x.shape for x in v]}") from None
    out = np.zeros((v[0].shape[0], 12), np.float32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11] = v
    return out


def quad_triangles(center, u, v):
    """The parallelogram center +- u +- v as two TRI12 records that share its diagonal: (2, 12) float32, (c - u - v, c + u - v, c + u + v)
    and (c - u - v, c + u + v, c - u + v), the corners computed in float64 and rounded once, both wound about cross(u, v)."""
    c, u, v = (np.asarray(x, np.float64).reshape(-1) for x in (center, u, v))
    if c.shape != (3,) or u.shape != (3,) or v.shape != (3,) or not (np.isfinite(c).all() and np.isfinite(u).all() and np.isfinite(v).all()):
        raise PtError(f"quad_triangles: want three finite vectors of 3 floats, got {center!r} {u!r} {v!r}")
    p00, p10, p11, p01 = c - u - v, c + u - v, c + u + v, c - u + v
    return tri_records([p00, p00], [p10, p11], [p11, p01])


def slice_triangles(point, normal, half_extent):
    """The two TRI12 records Scene.slice cuts the scene with: the square of that half-extent centred on `point` in the plane with that
    normal, its sides along u = normalize(cross(n, e)), e the axis on which n is smallest, and cross(n, u) (float64, rounded once)."""
    n = np.asarray(normal, np.float64).reshape(-1)
    if n.shape != (3,) or not np.isfinite(n).all() or not (n * n).sum() > 0 or not (np.isfinite(half_extent) and half_extent > 0):
        raise PtError(f"slice: want a finite non-zero normal of 3 floats and a half_extent > 0, got {normal!r} {half_extent!r}")
    n = n / np.sqrt((n * n).sum())
    u = np.cross(n, np.eye(3)[int(np.argmin(np.abs(n)))])
    u /= np.sqrt((u * u).sum())
    return quad_triangles(point, u * half_extent, np.cross(n, u) * half_extent)


def aabb_planes(lo, hi):
    """The six planes of the axis-aligned box [lo, hi]: (6, 4) float32, normals +e_k, -e_k per axis, d = hi_k, -lo_k: the coordinates
    themselves, so that a float32 box gives its own faces."""
    lo, hi = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,):
        raise PtError(f"aabb_planes: want lo and hi of 3 floats each, got {lo.shape} {hi.shape}")
    out = np.zeros((6, 4), np.float32)
    for k in range(3):
        out[2 * k, k], out[2 * k, 3] = 1, hi[k]
        out[2 * k + 1, k], out[2 * k + 1, 3] = -1, -lo[k]
    return out


def list_offsets(count, stream_ptr=0):
    """CSR offsets of per-query counts (include/pt_api.h: pt_list_offsets): (n + 1,) int64, offsets[0] = 0 and offsets[i + 1] =
    offsets[i] + max(count[i], 0), without wrapping at 2^31.  count: a contiguous int32 torch tensor of shape (n,) on a GPU, used in
    place: the scan is enqueued on stream_ptr on count's device and the offsets are a torch tensor there, valid once the stream has
    passed the scan.  A numpy array is scanned on device 0 through the NULL stream, with a wait, and the offsets come back as numpy."""
    import torch
    if isinstance(count, np.ndarray):
        c = np.ascontiguousarray(count)
        if c.dtype != np.int32 or c.ndim != 1:
            raise PtError(f"list_offsets: count must be int32 of shape (n,), got {c.dtype} {c.shape}")
        off = list_offsets(torch.from_numpy(c).to("cuda:0"))
        torch.cuda.synchronize(0)
        return off.cpu().numpy()
    if not (hasattr(count, "data_ptr") and hasattr(count, "is_contiguous")):
        raise PtError("list_offsets: count must be a torch tensor or a numpy array")
    if str(count.dtype) != "torch.int32" or not count.is_contiguous() or count.dim() != 1:
        raise PtError(f"list_offsets: count must be contiguous int32 of shape (n,), got {count.dtype} {tuple(count.shape)}")
    if count.device.type != "cuda":
        raise PtError(f"list_offsets: count is on {count.device}, want a GPU")
    n = count.shape[0]
    sb = lib().pt_list_offsets_scratch_bytes(n)
    with torch.cuda.device(count.device):
        off = torch.empty(n + 1, dtype=torch.int64, device=count.device)
        scratch = torch.empty(max(sb, 8), dtype=torch.uint8, device=count.device)
        cptr = count.data_ptr() or scratch.data_ptr()      # an empty tensor has no address; n = 0 reads no count
        _check(lib().pt_list_offsets(C.c_void_p(cptr), n, C.c_void_p(off.data_ptr()), C.c_void_p(scratch.data_ptr()), C.c_void_p(stream_ptr)),
               "pt_list_offsets")
        st = torch.cuda.ExternalStream(stream_ptr, device=count.device) if stream_ptr else torch.cuda.default_stream(count.device)
        if st.cuda_stream != torch.cuda.current_stream().cuda_stream:      # the NULL stream included
            scratch.record_stream(st)      # not reused before the stream the scan is on has passed it
    return off


def _read_total(off, stream_ptr):
    """off[-1] as an int: one 8-byte read-back on stream_ptr (or the NULL stream), which waits for that stream."""
    import torch
    st = torch.cuda.ExternalStream(stream_ptr, device=off.device) if stream_ptr else torch.cuda.default_stream(off.device)
    with torch.cuda.stream(st):
        return int(off[-1].item())


def tiles_floats(cam, prm):
    n = lib().pt_tiles_floats(C.byref(cam), C.byref(prm))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def work_bytes(cam, prm):
    n = lib().pt_work_bytes(C.byref(cam), C.byref(prm))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def untile(d_gathered_ptr, cam, world, d_frame_ptr, stream_ptr=0):
    _check(lib().pt_untile(C.c_void_p(d_gathered_ptr), C.byref(cam), world, C.c_void_p(d_frame_ptr), C.c_void_p(stream_ptr)), "pt_untile")


def untile_views(d_tiles_ptr, cam0, n_views, d_frames_ptr, stream_ptr=0):
    """pt_untile_views on raw device pointers: the view-major tile buffer of render_views_device -> (n_views, H, W, 3) frames, one launch."""
    _check(lib().pt_untile_views(C.c_void_p(d_tiles_ptr), C.byref(cam0), int(n_views), C.c_void_p(d_frames_ptr), C.c_void_p(stream_ptr)), "pt_untile_views")


def _camera_array(cams):
    if isinstance(cams, C.Array):
        return cams
    cams = list(cams)
    if not cams:
        raise PtError("a batch of views holds at least one camera")
    return (PtCamera * len(cams))(*cams)


def _first_passes(first_pass, n):
    if first_pass is None:
        return None
    fp = np.ascontiguousarray(first_pass, np.int32).reshape(-1)
    if fp.size != n:
        raise PtError(f"first_pass has {fp.size} entries for {n} views")
    return fp


def views_floats(cam, n_views):
    n = lib().pt_views_floats(C.byref(cam), int(n_views))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def views_work_bytes(cam, prm, n_views):
    n = lib().pt_views_work_bytes(C.byref(cam), C.byref(prm), int(n_views))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def rays_floats(n_rays):
    n = lib().pt_rays_floats(int(n_rays))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def rays_work_bytes(prm, n_rays):
    n = lib().pt_rays_work_bytes(C.byref(prm), int(n_rays))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def camera_rays(cam, pass_index, device=0):
    """The rays a camera's pass casts, for Scene.render_rays: (rays (H * W, 8) float32 in pixel order, row-major, seeds (H * W,) int32,
    seed_stride).  Directions are the jittered ones of that pass (pt_dbg_pixel_dir, on the GPU), seeds are py * W + px and the stride is
    W * H, so render_rays(rays, params(passes=1, first_pass=pass_index), seeds, seed_stride) is that pass of render(cam, ...) bit for bit."""
    W, H = cam.W, cam.H
    py, px = np.divmod(np.arange(W * H, dtype=np.int32), np.int32(W))
    out8 = dbg_pixel_dir(cam, np.stack([px, py, np.full(W * H, int(pass_index), np.int32)], 1), device)
    rays = np.zeros((W * H, 8), np.float32)
    rays[:, 0:3] = np.array(cam.pos[:], np.float32)
    rays[:, 3:6] = out8[:, 2:5]
    rays[:, 7] = 999999.0
    return rays, (py * np.int32(W) + px).astype(np.int32), W * H


def equirect_rays(pos, W, H):
    """A 360 x 180 degree panorama from `pos` as (H * W, 8) float32 RAY8 records, row-major.  Pixel (x, y) looks along azimuth
    phi = 2 pi (x + 0.5 - W / 2) / W and polar angle theta = pi (y + 0.5) / H from +y: direction (sin theta sin phi, cos theta,
    -sin theta cos phi), of unit length.  The middle of the image looks down -z (exactly the centre pixel when W and H are odd), x grows
    to the right (+x), row 0 is nearest +y.  tmax = 999999, the camera path's."""
    W, H = int(W), int(H)
    if W < 1 or H < 1:
        raise PtError(f"equirect_rays: {W}x{H}")
    phi = 2.0 * np.pi * (np.arange(W, dtype=np.float64) + 0.5 - W / 2.0) / W
    theta = np.pi * (np.arange(H, dtype=np.float64) + 0.5) / H
    st, ct = np.sin(theta)[:, None], np.cos(theta)[:, None]
    d = np.stack([st * np.sin(phi)[None, :], np.broadcast_to(ct, (H, W)), -st * np.cos(phi)[None, :]], -1)
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    rays = np.zeros((H * W, 8), np.float32)
    rays[:, 0:3] = np.asarray(pos, np.float32).reshape(3)
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 7] = 999999.0
    return rays


def _tile_list(tiles):
    return np.ascontiguousarray(tiles, np.int32).reshape(-1)


def tiles_of_window(cam, window):
    """Global numbers (row-major over the full frame, ascending) of the 8x8 tiles that overlap the half-open pixel window
    (x0, y0, x1, y1); raises for a window that is empty or not inside the frame."""
    x0, y0, x1, y1 = (int(v) for v in window)
    n = lib().pt_tiles_of_window(C.byref(cam), x0, y0, x1, y1, None, 0)
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    out = np.zeros(n, np.int32)
    lib().pt_tiles_of_window(C.byref(cam), x0, y0, x1, y1, _ptr(out), n)
    return out


def tile_list_floats(n_tiles):
    n = lib().pt_tile_list_floats(int(n_tiles))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def tile_list_work_bytes(cam, prm, n_tiles):
    n = lib().pt_tile_list_work_bytes(C.byref(cam), C.byref(prm), int(n_tiles))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def untile_list(d_tiles_ptr, tiles, cam, window, d_out_ptr, stream_ptr=0):
    """Scatter a list-major tile buffer into the row-major buffer of a window of the frame (raw device pointers); pixels of the
    window that no listed tile covers are left as they are (include/pt_api.h: pt_untile_list)."""
    t = _tile_list(tiles)
    x0, y0, x1, y1 = (int(v) for v in window)
    _check(lib().pt_untile_list(C.c_void_p(d_tiles_ptr), _ptr(t), t.size, C.byref(cam), x0, y0, x1, y1, C.c_void_p(d_out_ptr),
                                C.c_void_p(stream_ptr)), "pt_untile_list")


def aov_floats(cam):
    n = lib().pt_aov_floats(C.byref(cam))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def denoise_params(**kw):
    """PtDenoiseParams: pt_denoise_params_default, then the given fields (iterations, sigma_color, sigma_normal, sigma_depth,
    demodulate)."""
    p = PtDenoiseParams()
    lib().pt_denoise_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown denoise parameter {k}")
        setattr(p, k, v)
    return p


def denoise_work_bytes(W, H):
    n = lib().pt_denoise_work_bytes(W, H)
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def denoise(rgb, aov, sample_cnt, device=0, **params):
    """pt_denoise_host: (H, W, 3) frame as Scene.render returns it + (H, W, 8) AOVs -> denoised (H, W, 3) float32 of the same scale."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    H, W = rgb.shape[:2]
    if rgb.shape != (H, W, 3) or aov.shape != (H, W, AOV_FLOATS):
        raise ValueError(f"shapes {rgb.shape} / {aov.shape}: want (H, W, 3) and (H, W, {AOV_FLOATS})")
    out = np.zeros_like(rgb)
    p = denoise_params(**params)
    _check(lib().pt_denoise_host(device, _ptr(rgb), _ptr(aov), W, H, int(sample_cnt), C.byref(p), _ptr(out)), "pt_denoise_host")
    return out


def denoise_device(d_rgb_ptr, d_aov_ptr, W, H, sample_cnt, d_out_ptr, d_work_ptr, stream_ptr=0, **params):
    """pt_denoise on raw device pointers (d_work: denoise_work_bytes(W, H) bytes), enqueued on the given stream."""
    p = denoise_params(**params)
    _check(lib().pt_denoise(C.c_void_p(d_rgb_ptr), C.c_void_p(d_aov_ptr), W, H, int(sample_cnt), C.byref(p), C.c_void_p(d_out_ptr),
                            C.c_void_p(d_work_ptr), C.c_void_p(stream_ptr)), "pt_denoise")


def aov_window_floats(cam, window):
    x0, y0, x1, y1 = (int(v) for v in window)
    n = lib().pt_aov_window_floats(C.byref(cam), x0, y0, x1, y1)
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def aov_views_floats(cam, n_views):
    n = lib().pt_aov_views_floats(C.byref(cam), int(n_views))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def denoise_batch_work_bytes(W, H, n_frames):
    n = lib().pt_denoise_batch_work_bytes(W, H, int(n_frames))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def denoise_batch(rgb, aov, sample_cnt, device=0, **params):
    """pt_denoise_batch_host: (n, H, W, 3) frames of one size + (n, H, W, 8) AOVs -> denoised (n, H, W, 3) float32; slice k is bit for bit
    denoise(rgb[k], aov[k], sample_cnt, **params)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    aov = np.ascontiguousarray(aov, np.float32)
    if rgb.ndim != 4 or rgb.shape[3] != 3 or aov.shape != rgb.shape[:3] + (AOV_FLOATS,):
        raise ValueError(f"shapes {rgb.shape} / {aov.shape}: want (n, H, W, 3) and (n, H, W, {AOV_FLOATS})")
    n, H, W = rgb.shape[:3]
    out = np.zeros_like(rgb)
    p = denoise_params(**params)
    _check(lib().pt_denoise_batch_host(device, _ptr(rgb), _ptr(aov), W, H, n, int(sample_cnt), C.byref(p), _ptr(out)), "pt_denoise_batch_host")
    return out


def denoise_batch_device(d_rgb_ptr, d_aov_ptr, W, H, n_frames, sample_cnt, d_out_ptr, d_work_ptr, stream_ptr=0, **params):
    """pt_denoise_batch on raw device pointers (d_work: denoise_batch_work_bytes(W, H, n_frames) bytes), enqueued on the given stream."""
    p = denoise_params(**params)
    _check(lib().pt_denoise_batch(C.c_void_p(d_rgb_ptr), C.c_void_p(d_aov_ptr), W, H, int(n_frames), int(sample_cnt), C.byref(p),
                                  C.c_void_p(d_out_ptr), C.c_void_p(d_work_ptr), C.c_void_p(stream_ptr)), "pt_denoise_batch")


def denoise_margin(iterations=None):
    """pt_denoise_margin: how far (in x and in y) a pixel of the filter with that many iterations looks, 2 * (2^L - 1); None: the default L."""
    m = lib().pt_denoise_margin(denoise_params().iterations if iterations is None else int(iterations))
    if m < 0:
        raise PtError(lib().pt_last_error().decode())
    return m


def expand_window(cam, window, margin=-1):
    """pt_window_expand: the half-open window (x0, y0, x1, y1) grown by `margin` pixels on every side (-1: denoise_margin of the default
    iterations) and clipped to the frame, as a tuple."""
    w, out = (C.c_int32 * 4)(*(int(v) for v in window)), (C.c_int32 * 4)()
    _check(lib().pt_window_expand(C.byref(cam), C.byref(w), int(margin), C.byref(out)), "pt_window_expand")
    return tuple(out[:])


def _estimate_dict(e):
    return dict(rel_rms=e.rel_rms, mean_rel_se=e.mean_rel_se, pixels=e.pixels, skipped=e.skipped)


def accumulate_passes(d_work_ptr, cam, prm, n_before, d_sum_ptr, d_m2_ptr, stream_ptr=0):
    """pt_accumulate_passes on raw device pointers: folds the prm.passes per-pass means the last render_tiles(cam, prm, ..., d_work)
    left in d_work into the running moments S, M2 (tiles_floats(cam, prm) floats each); n_before = passes folded in so far."""
    _check(lib().pt_accumulate_passes(C.c_void_p(d_work_ptr), C.byref(cam), C.byref(prm), int(n_before), C.c_void_p(d_sum_ptr),
                                      C.c_void_p(d_m2_ptr), C.c_void_p(stream_ptr)), "pt_accumulate_passes")


def variance(d_m2_ptr, n_floats, n_passes, d_var_ptr, stream_ptr=0):
    """pt_variance on raw device pointers: d_var = max(M2, 0) * n / (n - 1), the estimated variance of S."""
    _check(lib().pt_variance(C.c_void_p(d_m2_ptr), int(n_floats), int(n_passes), C.c_void_p(d_var_ptr), C.c_void_p(stream_ptr)), "pt_variance")


def error_scratch_bytes(n_floats):
    n = lib().pt_error_scratch_bytes(int(n_floats))
    if n < 0:
        raise PtError(lib().pt_last_error().decode())
    return n


def error_estimate(d_sum_ptr, d_m2_ptr, cam, prm, n_passes, d_scratch_ptr, stream_ptr=0):
    """pt_error_estimate on raw device pointers (d_scratch: error_scratch_bytes(tiles_floats(cam, prm)) bytes); waits for the
    stream.  Returns dict(rel_rms, mean_rel_se, pixels, skipped)."""
    e = PtErrorEstimate()
    _check(lib().pt_error_estimate(C.c_void_p(d_sum_ptr), C.c_void_p(d_m2_ptr), C.byref(cam), C.byref(prm), int(n_passes),
                                   C.c_void_p(d_scratch_ptr), C.byref(e), C.c_void_p(stream_ptr)), "pt_error_estimate")
    return _estimate_dict(e)


def accumulate_tile_list(d_work_ptr, cam, prm, d_list_ptr, n_tiles, n_before, d_sum_ptr, d_m2_ptr, d_tile_passes_ptr=0, stream_ptr=0):
    """pt_accumulate_tile_list on raw device pointers: folds the prm.passes per-pass means a render_tile_list_device of n_tiles tiles left
    in d_work into the frame-layout moments S, M2 (tiles_floats(cam, world 1) floats each), list entry i into tile d_list[i] (int32 on the
    device); n_before = passes the listed tiles hold so far; d_tile_passes (0 = none): int32 per tile, set to n_before + prm.passes."""
    _check(lib().pt_accumulate_tile_list(C.c_void_p(d_work_ptr), C.byref(cam), C.byref(prm), C.c_void_p(d_list_ptr), int(n_tiles), int(n_before),
                                         C.c_void_p(d_sum_ptr), C.c_void_p(d_m2_ptr), C.c_void_p(d_tile_passes_ptr or None), C.c_void_p(stream_ptr)),
           "pt_accumulate_tile_list")


def tile_errors(d_sum_ptr, d_m2_ptr, cam, d_list_ptr, n_tiles, n_passes, d_err_ptr, stream_ptr=0):
    """pt_tile_errors on raw device pointers: one 16-byte PtTileError (TILE_ERROR_DTYPE) per list entry into d_err; d_list_ptr 0 = the
    tiles 0 .. n_tiles - 1 in order."""
    _check(lib().pt_tile_errors(C.c_void_p(d_sum_ptr), C.c_void_p(d_m2_ptr), C.byref(cam), C.c_void_p(d_list_ptr or None), int(n_tiles),
                                int(n_passes), C.c_void_p(d_err_ptr), C.c_void_p(stream_ptr)), "pt_tile_errors")


def finish_tiles(d_sum_ptr, d_m2_ptr, d_tile_passes_ptr, cam, d_mean_ptr=0, d_var_ptr=0, stream_ptr=0):
    """pt_finish_tiles on raw device pointers: mean = S / n and variance of S per tile's own pass count n (frame tile layout; either
    output may be 0, not both)."""
    _check(lib().pt_finish_tiles(C.c_void_p(d_sum_ptr), C.c_void_p(d_m2_ptr), C.c_void_p(d_tile_passes_ptr), C.byref(cam),
                                 C.c_void_p(d_mean_ptr or None), C.c_void_p(d_var_ptr or None), C.c_void_p(stream_ptr)), "pt_finish_tiles")


class Comm:
    """PtComm: the C-ABI's communicator for the single gather (RCCL under it when world > 1)."""

    def __init__(self, rank=0, world=1, device=0, unique_id=None, id_file=None, timeout_s=60, job_tag=0):
        self._h = C.c_void_p()
        if id_file is not None:
            _check(lib().pt_comm_create_from_file_tagged(id_file.encode(), job_tag, rank, world, device, timeout_s, C.byref(self._h)), "pt_comm_create_from_file_tagged")
        else:
            buf = (C.c_uint8 * 128)(*(unique_id or bytes(128)))
            _check(lib().pt_comm_create(buf, rank, world, device, C.byref(self._h)), "pt_comm_create")

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        _check(lib().pt_comm_unique_id(buf), "pt_comm_unique_id")
        return bytes(buf)

    @property
    def rank(self):
        return lib().pt_comm_rank(self._h)

    @property
    def world(self):
        return lib().pt_comm_world(self._h)

    def gather_tiles(self, d_tiles_ptr, n_floats, d_gathered_ptr, stream_ptr=0):
        _check(lib().pt_gather_tiles(self._h, C.c_void_p(d_tiles_ptr), n_floats, C.c_void_p(d_gathered_ptr), C.c_void_p(stream_ptr)), "pt_gather_tiles")

    def gather_frame(self, d_tiles_ptr, cam, prm, d_gathered_ptr, d_frame_ptr, stream_ptr=0):
        _check(lib().pt_gather_frame(self._h, C.c_void_p(d_tiles_ptr), C.byref(cam), C.byref(prm), C.c_void_p(d_gathered_ptr),
                                     C.c_void_p(d_frame_ptr), C.c_void_p(stream_ptr)), "pt_gather_frame")

    def render_split(self, scene, cam, prm):
        """pt_render_split: this rank's share + the gather; returns the (H, W, 3) frame on rank 0, None elsewhere."""
        out = np.zeros((cam.H, cam.W, 3), np.float32) if self.rank == 0 else None
        _check(lib().pt_render_split(scene.handle, C.byref(cam), C.byref(prm), self._h, _ptr(out) if out is not None else None), "pt_render_split")
        return out

    def close(self):
        if self._h:
            lib().pt_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dbg_bxdf(lobe, in28, device=0):
    in28 = np.ascontiguousarray(in28, np.float32).reshape(-1, 28)
    out = np.zeros((in28.shape[0], 12), np.float32)
    _check(lib().pt_dbg_bxdf(device, lobe, _ptr(in28), in28.shape[0], _ptr(out)), "pt_dbg_bxdf")
    return out


def dbg_rng(seed, n, device=0):
    raw = np.zeros(n, np.uint32)
    uni = np.zeros(n, np.float32)
    _check(lib().pt_dbg_rng(device, seed, n, _ptr(raw), _ptr(uni)), "pt_dbg_rng")
    return raw, uni


def triad_gbps(bytes_per_array=1 << 30, iters=10, device=0):
    """Measured streaming bandwidth of this GPU (float4 triad, 2 reads + 1 write), GB/s."""
    out = C.c_double(0.0)
    _check(lib().pt_dbg_triad(int(device), int(bytes_per_array), int(iters), C.byref(out)), "pt_dbg_triad")
    return float(out.value)


def valu_rate(op=0, waves_per_simd=4, iters=20000, device=0):
    """Measured VALU issue rate: (wave-instructions per second chip-wide, shader clock in GHz) for one instruction kind
    or short instruction group (pt_dbg_valu_rate: 0 v_fma_f32, 1 v_pk_fma_f32, 2 v_max3_f32, 3 v_cvt_f32_ubyte1, 4 v_add_u32,
    5 v_fma_f64, 6 v_cndmask_b32, 7 v_pk_mul_f32, 8..67: the table in tools/valu_probe.py; 16 = op 0 with half the lanes masked
    off, op + 256 = any op with half the lanes masked off)."""
    r, g = C.c_double(0.0), C.c_double(0.0)
    _check(lib().pt_dbg_valu_rate(int(device), int(op), int(waves_per_simd), int(iters), C.byref(r), C.byref(g)), "pt_dbg_valu_rate")
    return float(r.value), float(g.value)


def dbg_pixel_dir(cam, pxpypass, device=0):
    a = np.ascontiguousarray(pxpypass, np.int32).reshape(-1, 3)
    out = np.zeros((a.shape[0], 8), np.float32)
    _check(lib().pt_dbg_pixel_dir(device, C.byref(cam), _ptr(a), a.shape[0], _ptr(out)), "pt_dbg_pixel_dir")
    return out


def dbg_ray_setup(dirs, device=0):
    """wf_trace's per-ray set-up on (n, 3) directions -> (n, 5): Normalize(inv(dir)) xyz, cull scale, degenerate flag."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out = np.zeros((d.shape[0], 5), np.float32)
    _check(lib().pt_dbg_ray_setup(device, _ptr(d), d.shape[0], _ptr(out)), "pt_dbg_ray_setup")
    return out


def dbg_sincos(x, device=0):
    """(n, 2) float32: sin, cos of the samplers' device function (angles in [0, 2 pi])."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], 2), np.float32)
    _check(lib().pt_dbg_sincos(device, _ptr(x), x.shape[0], _ptr(out)), "pt_dbg_sincos")
    return out


def dbg_math(x, device=0):
    x = np.ascontiguousarray(x, np.float32).ravel()
    out = np.zeros((x.size, 8), np.float32)
    _check(lib().pt_dbg_math(device, _ptr(x), x.size, _ptr(out)), "pt_dbg_math")
    return out
