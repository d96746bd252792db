"""raytracer-utah_amd — MI355X-native render hot path for RayTracer-Utah scenes.

Python here is plumbing only (tests, bench.py, torch.distributed glue): a ctypes
view of the two product libraries

  lib/librtu_hip.so   C-ABI of include/rtu_render.h  (hand-written gfx950 HIP kernels)
  lib/librtu_host.so  C entry points of include/rtu_host.h (scene loader, flattener,
                      RenderImage mirror, PNG, BeginRender)

There is NO CPU fallback: if the HIP library is missing or cannot be loaded the
import fails loudly (build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C raytracer-utah_amd`). The CPU oracle lives under oracle/ and is test
infrastructure; nothing in this package touches it.

The directory name contains a hyphen, so it is imported by path as module
`raytracer_utah_amd` (see __graft_entry__.load_package()).
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_PKG, "lib")

RTU_BIGFLOAT = 1.0e30
RTU_BAND_ROWS = 8

RTU_OK = 0
RTU_ERR_ARG = -1
RTU_ERR_HIP = -2
RTU_ERR_UNSUPPORTED = -3
RTU_ERR_STOCHASTIC = -4
RTU_ERR_NO_SCENE = -5
RTU_ERR_NO_DEVICE = -6
RTU_ERR_CAPACITY = -7
RTU_ERR_CANCELLED = -8
RTU_ERR_SCENE_SHAPE = -9
RTU_ERR_STALE = -10  # a progressive session's context got a new scene


class RtuError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        if code == RTU_ERR_SCENE_SHAPE:
            msg = "scene shape differs from the uploaded scene: " + msg
        super().__init__("rtu error %d: %s" % (code, msg))


class RtuCamera(ctypes.Structure):
    _fields_ = [("pos", ctypes.c_float * 3), ("dir", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
                ("fov", ctypes.c_float), ("focaldist", ctypes.c_float), ("dof", ctypes.c_float),
                ("img_width", ctypes.c_int32), ("img_height", ctypes.c_int32)]


class RtuEnvColor(ctypes.Structure):
    _fields_ = [("color", ctypes.c_float * 3), ("has_map", ctypes.c_int32), ("map_is_null", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


class RtuTexMap(ctypes.Structure):
    _fields_ = [("present", ctypes.c_int32), ("texture", ctypes.c_int32), ("tm", ctypes.c_float * 9), ("itm", ctypes.c_float * 9),
                ("pos", ctypes.c_float * 3), ("reserved", ctypes.c_int32)]


class RtuMesh(ctypes.Structure):
    _fields_ = [("nv", ctypes.c_uint32), ("nf", ctypes.c_uint32), ("nvn", ctypes.c_uint32), ("nvt", ctypes.c_uint32),
                ("n_bvh_nodes", ctypes.c_uint32), ("n_elements", ctypes.c_uint32), ("bvh_depth", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("bound_min", ctypes.c_float * 3), ("bound_max", ctypes.c_float * 3),
                ("v", ctypes.c_void_p), ("f", ctypes.c_void_p), ("vn", ctypes.c_void_p), ("fn", ctypes.c_void_p),
                ("vt", ctypes.c_void_p), ("ft", ctypes.c_void_p), ("bvh", ctypes.c_void_p), ("elements", ctypes.c_void_p)]


class RtuSceneDesc(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint32), ("n_materials", ctypes.c_uint32), ("n_lights", ctypes.c_uint32),
                ("n_meshes", ctypes.c_uint32), ("nodes", ctypes.c_void_p), ("materials", ctypes.c_void_p),
                ("lights", ctypes.c_void_p), ("meshes", ctypes.c_void_p), ("camera", RtuCamera),
                ("background", RtuEnvColor), ("environment", RtuEnvColor),
                ("n_textures", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("textures", ctypes.c_void_p),
                ("material_maps", ctypes.c_void_p), ("background_map", RtuTexMap), ("environment_map", RtuTexMap)]


class RtuFrameDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("shard_rank", ctypes.c_int32),
                ("shard_count", ctypes.c_int32), ("max_bounce", ctypes.c_int32), ("collect_stats", ctypes.c_int32),
                ("coop_threshold", ctypes.c_int32), ("samples", ctypes.c_int32), ("cam_pos", ctypes.c_float * 3), ("origin", ctypes.c_float * 3),
                ("u", ctypes.c_float * 3), ("v", ctypes.c_float * 3), ("lens_up", ctypes.c_float * 3), ("lens_right", ctypes.c_float * 3),
                ("dof", ctypes.c_float), ("gather_bounces", ctypes.c_int32)]


STAT_FIELDS = ("primary_rays", "primary_hits", "secondary_rays", "shadow_rays", "node_tests", "mesh_entries",
               "inner_visits", "leaf_visits", "leaf_elems", "tri_tests", "tri_accepts")


class RtuStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in STAT_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in STAT_FIELDS}


TOUCH_FIELDS = ["rays", "node_tests", "mesh_box_tests", "inner4", "inner8", "inner_ref", "tri_tests", "winners", "xform_levels", "record_bytes", "bound_tests", "inline_shadow_rays"]
KERNEL_SLOTS = 40


class RtuTouched(ctypes.Structure):
    """rtu_render.h: what one kernel launch of the fast variant touched (collect_stats == 2)."""
    _fields_ = [(n, ctypes.c_uint64) for n in TOUCH_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in TOUCH_FIELDS}


def algorithmic_bytes(stats, pixels):
    """cache-agnostic bytes the path touches for one frame."""
    s = stats if isinstance(stats, dict) else stats.as_dict()
    return (56 * s["inner_visits"] + 4 * s["leaf_elems"] + 48 * s["tri_tests"] + 96 * s["tri_accepts"]
            + 72 * s["node_tests"] + 16 * pixels)


def total_rays(stats):
    s = stats if isinstance(stats, dict) else stats.as_dict()
    return s["primary_rays"] + s["secondary_rays"] + s["shadow_rays"]


def _load(name):
    path = os.path.join(_LIB, name)
    if not os.path.exists(path):
        raise ImportError("%s is missing: build the HIP extension first (__graft_entry__.build() or "
                          "`make -C raytracer-utah_amd`); there is no CPU fallback" % path)
    return ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


hip = _load("librtu_hip.so")
host = _load("librtu_host.so")

_P = ctypes.c_void_p
_I = ctypes.c_int


def _sig(lib, name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


# ---- rtu_render.h ----------------------------------------------------------
HIP_SYMBOLS = ["rtu_device_count", "rtu_error_string", "rtu_create_context", "rtu_destroy_context", "rtu_last_error",
               "rtu_upload_scene", "rtu_validate_scene", "rtu_frame_setup", "rtu_shard_rows", "rtu_shard_max_rows", "rtu_shard_global_row",
               "rtu_render_frame_device", "rtu_render_frames_device", "rtu_pack_image_device", "rtu_minmax_z_device", "rtu_pack_output_device", "rtu_render_frame", "rtu_frame_status", "rtu_render_timeline", "rtu_frame_counts", "rtu_timeline_exits", "rtu_mesh_info", "rtu_light_list_info", "rtu_debug_light_list", "rtu_update_scene", "rtu_multi_update_scene", "rtu_scene_shape_diff", "rtu_debug_context_light_list", "rtu_debug_update_timing", "rtu_debug_light_list_free", "rtu_debug_walk_stack_limit", "rtu_debug_node_bounds", "rtu_debug_flags", "rtu_set_sequences_in_flight", "rtu_debug_tail_from", "rtu_get_stats", "rtu_get_touched", "rtu_get_touched_launches", "rtu_touched_bytes", "rtu_kernel_slot_name", "rtu_probe_kernel", "rtu_probe_read", "rtu_time_render", "rtu_selftest_division", "rtu_selftest_primitives", "rtu_context_stream", "rtu_context_device", "rtu_context_sync", "rtu_host_alloc_pinned", "rtu_host_free_pinned", "rtu_copy_to_host_async", "rtu_device_alloc",
               "rtu_device_free", "rtu_copy_to_host", "rtu_device_info", "rtu_set_cancel_flag", "rtu_create_context_multi", "rtu_destroy_context_multi",
               "rtu_multi_size", "rtu_multi_context", "rtu_multi_last_error", "rtu_multi_upload_scene", "rtu_multi_render_frame", "rtu_multi_gather_kind",
               "rtu_adaptive_defaults", "rtu_render_frame_adaptive", "rtu_render_frame_adaptive_device", "rtu_debug_sample_images", "rtu_debug_texcoords",
               "rtu_debug_device_allocations", "rtu_progressive_begin", "rtu_progressive_advance", "rtu_progressive_status",
               "rtu_progressive_snapshot_device", "rtu_progressive_snapshot", "rtu_progressive_free", "rtu_debug_device_bytes",
               "rtu_update_meshes", "rtu_multi_update_meshes", "rtu_debug_context_mesh", "rtu_debug_host_mesh", "rtu_debug_mesh_update_timing",
               "rtu_update_meshes_device", "rtu_context_mesh_shape", "rtu_debug_host_ref_build", "rtu_debug_partition_rule",
               "rtu_debug_mesh_update_device_timing",
               "rtu_trace_rays_device", "rtu_occluded_rays_device", "rtu_trace_rays", "rtu_occluded_rays", "rtu_camera_rays",
               "rtu_shade_defaults", "rtu_shade_rays_device", "rtu_shade_rays",
               "rtu_shade_rays_sampled_device", "rtu_shade_rays_sampled", "rtu_camera_sample_rays", "rtu_sample_key", "rtu_child_key",
               "rtu_shade_rays_paths_device", "rtu_shade_rays_paths", "rtu_debug_last_tail_from",
               "rtu_ray_sort_box", "rtu_scene_sort_box", "rtu_ray_sort_keys", "rtu_ray_order_device", "rtu_ray_order", "rtu_permute_device", "rtu_copy_to_device",
               "rtu_sensor_defaults", "rtu_sensor_rays", "rtu_sensor_rays_device", "rtu_render_sensor", "rtu_render_sensor_device",
               "rtu_debug_sensor_timing",
               "rtu_render_sensor_adaptive", "rtu_render_sensor_adaptive_device", "rtu_debug_sensor_adaptive_trace",
               "rtu_ray_features_device", "rtu_ray_features", "rtu_frame_features_device", "rtu_frame_features",
               "rtu_ray_surface_device", "rtu_ray_surface", "rtu_frame_surface_device", "rtu_frame_surface",
               "rtu_keep_previous_vertices", "rtu_scene_motion_deform", "rtu_temporal_accumulate_deform", "rtu_temporal_accumulate_deform_moments",
               "rtu_temporal_accumulate_deform_device", "rtu_temporal_accumulate_deform_moments_device", "rtu_motion_vectors_deform",
               "rtu_motion_vectors_deform_device", "rtu_temporal_frame_deformed_device", "rtu_temporal_frame_deformed",
               "rtu_denoise_defaults", "rtu_denoise", "rtu_denoise_device",
               "rtu_progressive_snapshot_denoised_device", "rtu_progressive_snapshot_denoised",
               "rtu_camera_sample_rays_device", "rtu_temporal_defaults", "rtu_temporal_accumulate", "rtu_temporal_accumulate_device",
               "rtu_temporal_begin", "rtu_temporal_frame_device", "rtu_temporal_frame", "rtu_temporal_history_device", "rtu_temporal_reset",
               "rtu_temporal_free", "rtu_scene_motion", "rtu_temporal_accumulate_motion", "rtu_temporal_accumulate_motion_device",
               "rtu_motion_vectors", "rtu_motion_vectors_device", "rtu_temporal_frame_moved_device", "rtu_temporal_frame_moved",
               "rtu_variance_defaults", "rtu_temporal_accumulate_moments", "rtu_temporal_accumulate_moments_device", "rtu_variance",
               "rtu_variance_device", "rtu_denoise_variance", "rtu_denoise_variance_device", "rtu_temporal_begin_variance",
               "rtu_steer_defaults", "rtu_sample_allocation", "rtu_sample_allocation_device", "rtu_extra_sample_rays",
               "rtu_extra_sample_rays_device", "rtu_temporal_refine", "rtu_temporal_refine_device", "rtu_temporal_begin_steered",
               "rtu_temporal_extra_counts_device", "rtu_temporal_steer_total",
               "rtu_gradient_defaults", "rtu_gradient_rays", "rtu_gradient_rays_device", "rtu_sample_luminance", "rtu_sample_luminance_device",
               "rtu_temporal_gradient", "rtu_temporal_gradient_device", "rtu_temporal_accumulate_gradient",
               "rtu_temporal_accumulate_gradient_device", "rtu_temporal_begin_gradient", "rtu_temporal_lambda_device",
               "rtu_sparse_defaults", "rtu_sparse_rays", "rtu_sparse_rays_device", "rtu_temporal_accumulate_sparse",
               "rtu_temporal_accumulate_sparse_device", "rtu_sparse_fill", "rtu_sparse_fill_device", "rtu_temporal_begin_sparse",
               "rtu_temporal_holes",
               "rtu_hole_defaults", "rtu_hole_allocation", "rtu_hole_allocation_device", "rtu_hole_fold", "rtu_hole_fold_device",
               "rtu_temporal_begin_sparse_holes", "rtu_temporal_hole_rays",
               "rtu_sensor_project", "rtu_temporal_accumulate_sensor", "rtu_temporal_accumulate_sensor_device",
               "rtu_temporal_accumulate_sensor_moments", "rtu_temporal_accumulate_sensor_moments_device",
               "rtu_temporal_sensor_frame_device", "rtu_temporal_sensor_frame",
               "rtu_gather_rays_device", "rtu_gather_rays", "rtu_shade_rays_ambient_device", "rtu_shade_rays_ambient",
               "rtu_irradiance_defaults", "rtu_irradiance_grid", "rtu_irradiance_rays", "rtu_irradiance_classify", "rtu_irradiance_sample",
               "rtu_irradiance_sample_device", "rtu_irradiance_build_device", "rtu_irradiance_build",
               "rtu_render_frame_irradiance_device", "rtu_render_frame_irradiance"]
_sig(hip, "rtu_device_count", _I)
_sig(hip, "rtu_error_string", ctypes.c_char_p, _I)
_sig(hip, "rtu_create_context", _P, _I, ctypes.POINTER(_I))
_sig(hip, "rtu_destroy_context", None, _P)
_sig(hip, "rtu_last_error", ctypes.c_char_p, _P)
_sig(hip, "rtu_upload_scene", _I, _P, _P)
_sig(hip, "rtu_validate_scene", _I, _P, ctypes.c_char_p, ctypes.c_size_t)
_sig(hip, "rtu_frame_setup", _I, ctypes.POINTER(RtuCamera), _I, _I, ctypes.POINTER(RtuFrameDesc))
_sig(hip, "rtu_shard_rows", _I, ctypes.POINTER(RtuFrameDesc))
_sig(hip, "rtu_shard_max_rows", _I, _I, _I)
_sig(hip, "rtu_shard_global_row", _I, ctypes.POINTER(RtuFrameDesc), _I)
_sig(hip, "rtu_render_frame_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _P)
_sig(hip, "rtu_render_frames_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _I, _P, _P)
_sig(hip, "rtu_pack_image_device", _I, _P, _P, ctypes.c_size_t, _P, _P, _P)
_sig(hip, "rtu_minmax_z_device", _I, _P, _P, ctypes.c_size_t, _I, _P, _P)
_sig(hip, "rtu_pack_output_device", _I, _P, _P, ctypes.c_size_t, _I, _P, _P, _P)
_sig(hip, "rtu_render_frame", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, ctypes.POINTER(RtuStats))
_sig(hip, "rtu_frame_status", _I, _P)
_sig(hip, "rtu_get_touched", _I, _P, ctypes.POINTER(RtuTouched), _I)
_sig(hip, "rtu_touched_bytes", ctypes.c_uint64, ctypes.POINTER(RtuTouched), _I)
_sig(hip, "rtu_get_touched_launches", _I, _P, ctypes.POINTER(ctypes.c_uint32), _I)
_sig(hip, "rtu_kernel_slot_name", ctypes.c_char_p, _I)
_sig(hip, "rtu_probe_kernel", _I, _P, _I)
_sig(hip, "rtu_probe_read", _I, _P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_I))
_sig(hip, "rtu_debug_walk_stack_limit", _I, _P, ctypes.c_uint32)
_sig(hip, "rtu_debug_node_bounds", _I, _P, _I)
_sig(hip, "rtu_debug_flags", _I, _P, ctypes.c_uint32)
_sig(hip, "rtu_set_sequences_in_flight", _I, _P, _I)
_sig(hip, "rtu_debug_tail_from", _I, _P, _I)
_sig(hip, "rtu_debug_last_tail_from", _I, _P)
_sig(hip, "rtu_timeline_exits", _I, _P, _I, _I, ctypes.POINTER(ctypes.c_double))
_sig(hip, "rtu_mesh_info", _I, _P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32))
_sig(hip, "rtu_light_list_info", _I, _P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32))
_sig(hip, "rtu_frame_counts", _I, _P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32))
_sig(hip, "rtu_render_timeline", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _I, ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_double),
     ctypes.POINTER(ctypes.c_double))
_sig(hip, "rtu_get_stats", _I, _P, ctypes.POINTER(RtuStats))
_sig(hip, "rtu_time_render", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _P, _I, ctypes.POINTER(ctypes.c_float))
_sig(hip, "rtu_selftest_primitives", _I, _P, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_ulonglong))
_sig(hip, "rtu_selftest_division", _I, _P, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_ulonglong))
_sig(hip, "rtu_device_alloc", _P, _P, ctypes.c_size_t)
_sig(hip, "rtu_device_free", None, _P, _P)
_sig(hip, "rtu_copy_to_host", _I, _P, _P, _P, ctypes.c_size_t)


class RtuAdaptiveDesc(ctypes.Structure):
    _fields_ = [("min_samples", ctypes.c_int32), ("increment", ctypes.c_int32), ("target_variance", ctypes.c_float), ("max_batch", ctypes.c_int32)]


RTU_MAX_BATCH = 16
_sig(hip, "rtu_adaptive_defaults", _I, ctypes.POINTER(RtuAdaptiveDesc))
_sig(hip, "rtu_render_frame_adaptive", _I, _P, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuAdaptiveDesc), _P, _P, ctypes.POINTER(RtuStats))
_sig(hip, "rtu_render_frame_adaptive_device", _I, _P, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuAdaptiveDesc), _P, _P, _P)
_sig(hip, "rtu_debug_sample_images", _I, _P, ctypes.POINTER(RtuFrameDesc), _I, _I, _P)
_sig(hip, "rtu_debug_texcoords", _I, _P, _I, _I, _P, ctypes.c_ulonglong, _P)
_sig(hip, "rtu_debug_device_allocations", ctypes.c_ulonglong)
_sig(hip, "rtu_debug_device_bytes", ctypes.c_ulonglong)
_sig(hip, "rtu_progressive_begin", _P, _P, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuAdaptiveDesc), ctypes.POINTER(_I))
_sig(hip, "rtu_progressive_advance", _I, _P, _I, _P)
_sig(hip, "rtu_progressive_status", _I, _P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32))
_sig(hip, "rtu_progressive_snapshot_device", _I, _P, _P, _P, _P)
_sig(hip, "rtu_progressive_snapshot", _I, _P, _P, _P)
_sig(hip, "rtu_progressive_free", None, _P)
# rtu_debug_texcoords operations (include/rtu_render.h RTU_TEXOP_*) and the floats per input / output of each
TEXOP_ATAN2F, TEXOP_ASINF, TEXOP_SPHERE_UV, TEXOP_ENV_UVW, TEXOP_TILE_CLAMP, TEXOP_TEXTURE, TEXOP_MAP = range(7)
TEXOP_IN = (2, 1, 3, 3, 3, 3, 3)
TEXOP_OUT = (1, 1, 3, 3, 3, 3, 3)


def adaptive_defaults(**overrides):
    """RtuAdaptiveDesc with the reference's constants (min_samples 8, increment 1, target_variance 0.005, max_batch 0), then `overrides`."""
    d = RtuAdaptiveDesc()
    rc = hip.rtu_adaptive_defaults(ctypes.byref(d))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_adaptive_defaults")
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


class RtuDeviceInfo(ctypes.Structure):
    _fields_ = [("compute_units", ctypes.c_int32), ("clock_khz", ctypes.c_int32), ("memory_clock_khz", ctypes.c_int32), ("memory_bus_bits", ctypes.c_int32),
                ("l2_bytes", ctypes.c_uint64), ("hbm_bytes", ctypes.c_uint64), ("name", ctypes.c_char * 64), ("arch", ctypes.c_char * 64)]


ROWS_DONE = ctypes.CFUNCTYPE(None, _P, ctypes.POINTER(ctypes.c_float), _I, _I)


class RtuProgress(ctypes.Structure):
    _fields_ = [("cancel", ctypes.POINTER(_I)), ("rows_done", ROWS_DONE), ("user", _P)]


_sig(hip, "rtu_device_info", _I, _I, ctypes.POINTER(RtuDeviceInfo))
_sig(hip, "rtu_set_cancel_flag", _I, _P, ctypes.POINTER(_I))
_sig(hip, "rtu_create_context_multi", _P, ctypes.POINTER(_I), _I, ctypes.POINTER(_I))
_sig(hip, "rtu_destroy_context_multi", None, _P)
_sig(hip, "rtu_multi_size", _I, _P)
_sig(hip, "rtu_multi_context", _P, _P, _I)
_sig(hip, "rtu_multi_last_error", ctypes.c_char_p, _P)
_sig(hip, "rtu_multi_upload_scene", _I, _P, _P)
_sig(hip, "rtu_multi_render_frame", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, ctypes.POINTER(RtuProgress))
_sig(hip, "rtu_multi_gather_kind", _I, _P)


class RtuLightListDump(ctypes.Structure):
    _fields_ = [("usable", ctypes.c_int32), ("node", ctypes.c_int32), ("light", ctypes.c_int32), ("G", ctypes.c_uint32), ("point", ctypes.c_uint32),
                ("n_entries", ctypes.c_uint32), ("X", ctypes.c_float * 3), ("Y", ctypes.c_float * 3), ("Z", ctypes.c_float * 3), ("L", ctypes.c_float * 3),
                ("u0", ctypes.c_float), ("v0", ctypes.c_float), ("su", ctypes.c_float), ("sv", ctypes.c_float),
                ("cell_off", ctypes.POINTER(ctypes.c_uint32)), ("entry_face", ctypes.POINTER(ctypes.c_uint32)), ("entry_zmin", ctypes.POINTER(ctypes.c_float))]


_sig(hip, "rtu_debug_light_list", _I, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(RtuLightListDump))
_sig(hip, "rtu_debug_light_list_free", None, ctypes.POINTER(RtuLightListDump))
_sig(hip, "rtu_update_scene", _I, _P, _P)
_sig(hip, "rtu_multi_update_scene", _I, _P, _P)
_sig(hip, "rtu_scene_shape_diff", _I, _P, _P, ctypes.c_char_p, ctypes.c_size_t)
_sig(hip, "rtu_debug_context_light_list", _I, _P, ctypes.c_uint32, ctypes.POINTER(RtuLightListDump))
_sig(hip, "rtu_debug_update_timing", _I, _P, _I, ctypes.POINTER(ctypes.c_float))
_sig(hip, "rtu_update_meshes", _I, _P, _P, ctypes.POINTER(ctypes.c_uint32), _I)
_sig(hip, "rtu_multi_update_meshes", _I, _P, _P, ctypes.POINTER(ctypes.c_uint32), _I)
_sig(hip, "rtu_debug_mesh_update_timing", _I, _P, _I, ctypes.POINTER(ctypes.c_float))
_sig(hip, "rtu_debug_context_mesh", _I, _P, ctypes.c_uint32, _I, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t))
_sig(hip, "rtu_debug_host_mesh", _I, _P, _P, _I, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t))


RTU_MESH_EDIT_RECOMPUTE_NORMALS = 1


class RtuMeshDeviceEdit(ctypes.Structure):
    _fields_ = [("mesh", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("d_v", ctypes.c_void_p), ("d_vn", ctypes.c_void_p)]


_sig(hip, "rtu_update_meshes_device", _I, _P, _P, _P, _I, _P)
_sig(hip, "rtu_context_mesh_shape", _I, _P, ctypes.c_uint32, ctypes.POINTER(RtuMesh))
_sig(hip, "rtu_debug_host_ref_build", _I, _P, _P, _I, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t))
_sig(hip, "rtu_debug_partition_rule", _I, _P, ctypes.c_uint32, _P)
_sig(hip, "rtu_debug_mesh_update_device_timing", _I, _P, ctypes.POINTER(ctypes.c_float))

# ray queries (include/rtu_render.h RtuRay / RtuRayHit): numpy layouts are built where numpy is imported (ray_dtype / hit_dtype)
RTU_RAY_HIT, RTU_RAY_FRONT, RTU_RAY_INVALID = 1, 2, 4
RTU_QUERY_REFERENCE_WALK = 1
_sig(hip, "rtu_trace_rays_device", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P, _P)
_sig(hip, "rtu_occluded_rays_device", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P, _P)
_sig(hip, "rtu_trace_rays", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P)
_sig(hip, "rtu_occluded_rays", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P)
_sig(hip, "rtu_camera_rays", _I, ctypes.POINTER(RtuFrameDesc), _I, _I, _P)


class RtuShadeDesc(ctypes.Structure):
    """include/rtu_render.h RtuShadeDesc (32 bytes): how a ray batch is shaded."""
    _fields_ = [("eye", ctypes.c_float * 3), ("max_bounce", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


_sig(hip, "rtu_shade_defaults", _I, ctypes.POINTER(RtuShadeDesc))
_sig(hip, "rtu_shade_rays_device", _I, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, _P)
_sig(hip, "rtu_shade_rays", _I, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, ctypes.POINTER(RtuStats))
_sig(hip, "rtu_shade_rays_sampled_device", _I, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, _P)
_sig(hip, "rtu_shade_rays_sampled", _I, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, ctypes.POINTER(RtuStats))
_sig(hip, "rtu_shade_rays_paths_device", _I, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, _P)
_sig(hip, "rtu_shade_rays_paths", _I, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, ctypes.POINTER(RtuStats))
_sig(hip, "rtu_camera_sample_rays", _I, ctypes.POINTER(RtuFrameDesc), _I, _I, _I, _P, _P)
_sig(hip, "rtu_gather_rays_device", _I, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, _P)
_sig(hip, "rtu_gather_rays", _I, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, ctypes.POINTER(RtuStats))
_sig(hip, "rtu_shade_rays_ambient_device", _I, _P, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, _P)
_sig(hip, "rtu_shade_rays_ambient", _I, _P, _P, _P, _P, ctypes.c_size_t, ctypes.POINTER(RtuShadeDesc), _P, ctypes.POINTER(RtuStats))


class RtuIrradianceDesc(ctypes.Structure):
    """include/rtu_render.h RtuIrradianceDesc (64 bytes): the grid, the samples per computed point and the thresholds of an irradiance map."""
    _fields_ = [("min_subdiv", ctypes.c_int32), ("max_subdiv", ctypes.c_int32), ("samples", ctypes.c_int32), ("first_sample", ctypes.c_int32),
                ("threshold_color", ctypes.c_float * 3), ("threshold_z", ctypes.c_float), ("threshold_n", ctypes.c_float),
                ("max_bounce", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 6)]


class RtuIrradianceMap(ctypes.Structure):
    """include/rtu_render.h RtuIrradianceMap (32 bytes): a built map for the lookup and the frame."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("max_subdiv", ctypes.c_int32), ("reserved", ctypes.c_uint32),
                ("records", ctypes.c_void_p), ("reserved_ptr", ctypes.c_void_p)]


_PI = ctypes.POINTER(_I)
_sig(hip, "rtu_irradiance_defaults", _I, ctypes.POINTER(RtuIrradianceDesc))
_sig(hip, "rtu_irradiance_grid", _I, ctypes.POINTER(RtuIrradianceDesc), _I, _I, _PI, _PI, _PI)
_sig(hip, "rtu_irradiance_rays", _I, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuIrradianceDesc), _P)
_sig(hip, "rtu_irradiance_classify", _I, ctypes.POINTER(RtuIrradianceDesc), _I, _I, _I, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_uint32))
_sig(hip, "rtu_irradiance_sample", _I, ctypes.POINTER(RtuIrradianceMap), _P, ctypes.c_size_t, _P)
_sig(hip, "rtu_irradiance_sample_device", _I, _P, ctypes.POINTER(RtuIrradianceMap), _P, ctypes.c_size_t, _P, _P)
_sig(hip, "rtu_irradiance_build_device", _I, _P, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuIrradianceDesc), _P, _P,
     ctypes.POINTER(ctypes.c_uint32), _P, _P)
_sig(hip, "rtu_irradiance_build", _I, _P, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuIrradianceDesc), _P, _P, ctypes.POINTER(ctypes.c_uint32), _P)
_sig(hip, "rtu_render_frame_irradiance_device", _I, _P, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuIrradianceMap), _P, _P)
_sig(hip, "rtu_render_frame_irradiance", _I, _P, ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuIrradianceMap), _P)
_sig(hip, "rtu_sample_key", ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
_sig(hip, "rtu_child_key", ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32)
# ray sorting (include/rtu_render.h, "Ray sorting")
RTU_SORTKEY_INVALID, RTU_SORTKEY_MISS = 0xFFFFFFFF, 0x40000000  # MISS: a bit, beside the 18 direction bits
_sig(hip, "rtu_ray_sort_box", _I, _P, ctypes.POINTER(ctypes.c_float))
_sig(hip, "rtu_scene_sort_box", _I, _P, ctypes.POINTER(ctypes.c_float))
_sig(hip, "rtu_ray_sort_keys", _I, ctypes.POINTER(ctypes.c_float), _P, ctypes.c_size_t, _P)
_sig(hip, "rtu_ray_order_device", _I, _P, _P, ctypes.c_size_t, _P, _P)
_sig(hip, "rtu_ray_order", _I, _P, _P, ctypes.c_size_t, _P)
_sig(hip, "rtu_permute_device", _I, _P, _P, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _I, _P)
_sig(hip, "rtu_copy_to_device", _I, _P, _P, _P, ctypes.c_size_t)
_sig(hip, "rtu_context_stream", _P, _P)
_sig(hip, "rtu_context_sync", _I, _P)


# sensors (include/rtu_render.h, "Sensors")
RTU_SENSOR_EQUIRECT, RTU_SENSOR_FISHEYE, RTU_SENSOR_ORTHO = 0, 1, 2
SENSOR_MODELS = {"equirect": RTU_SENSOR_EQUIRECT, "fisheye": RTU_SENSOR_FISHEYE, "ortho": RTU_SENSOR_ORTHO}


class RtuSensorDesc(ctypes.Structure):
    """include/rtu_render.h RtuSensorDesc (128 bytes): a panoramic, fisheye or orthographic sensor and how it is sampled."""
    _fields_ = [("model", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("samples", ctypes.c_int32),
                ("gather_bounces", ctypes.c_int32), ("max_bounce", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("pos", ctypes.c_float * 3), ("right", ctypes.c_float * 3), ("up", ctypes.c_float * 3), ("forward", ctypes.c_float * 3),
                ("fov_deg", ctypes.c_float), ("extent", ctypes.c_float * 2), ("reserved", ctypes.c_uint32 * 10)]


_sig(hip, "rtu_sensor_defaults", _I, ctypes.POINTER(RtuSensorDesc))
_sig(hip, "rtu_sensor_rays", _I, ctypes.POINTER(RtuSensorDesc), _I, _I, _I, _P, _P)
_sig(hip, "rtu_sensor_rays_device", _I, _P, ctypes.POINTER(RtuSensorDesc), _I, _I, _P, _P, _P)
_sig(hip, "rtu_render_sensor", _I, _P, ctypes.POINTER(RtuSensorDesc), _P)
_sig(hip, "rtu_render_sensor_device", _I, _P, ctypes.POINTER(RtuSensorDesc), _P, _P)
_sig(hip, "rtu_debug_sensor_timing", _I, _P, _I, ctypes.POINTER(ctypes.c_float))
# adaptive sensors (include/rtu_render.h, "Adaptive sensors")
_sig(hip, "rtu_render_sensor_adaptive", _I, _P, ctypes.POINTER(RtuSensorDesc), ctypes.POINTER(RtuAdaptiveDesc), _P, _P)
_sig(hip, "rtu_render_sensor_adaptive_device", _I, _P, ctypes.POINTER(RtuSensorDesc), ctypes.POINTER(RtuAdaptiveDesc), _P, _P, _P)
_sig(hip, "rtu_debug_sensor_adaptive_trace", _I, _P, _P, _P, _I)


# first-hit features and the denoising filter (include/rtu_render.h, "First-hit features", "Denoising")
class RtuDenoiseDesc(ctypes.Structure):
    """include/rtu_render.h RtuDenoiseDesc (32 bytes): the size of the image and the four constants of the filter."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("n_passes", ctypes.c_int32), ("sigma_color", ctypes.c_float),
                ("sigma_plane", ctypes.c_float), ("normal_log2_power", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 2)]


_sig(hip, "rtu_ray_features_device", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P, _P, _P)
_sig(hip, "rtu_ray_features", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P, _P)
_sig(hip, "rtu_frame_features_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _P, _P)
_sig(hip, "rtu_frame_features", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _P)
_sig(hip, "rtu_ray_surface_device", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P, _P, _P, _P)
_sig(hip, "rtu_ray_surface", _I, _P, _P, ctypes.c_size_t, ctypes.c_uint32, _P, _P, _P)
_sig(hip, "rtu_frame_surface_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _P, _P, _P)
_sig(hip, "rtu_frame_surface", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _P, _P)
_sig(hip, "rtu_denoise_defaults", _I, ctypes.POINTER(RtuDenoiseDesc))
_sig(hip, "rtu_denoise", _I, ctypes.POINTER(RtuDenoiseDesc), _P, _P, _P, _P)
_sig(hip, "rtu_denoise_device", _I, _P, ctypes.POINTER(RtuDenoiseDesc), _P, _P, _P, _P, _P)
_sig(hip, "rtu_progressive_snapshot_denoised_device", _I, _P, ctypes.POINTER(RtuDenoiseDesc), _P, _P)
_sig(hip, "rtu_progressive_snapshot_denoised", _I, _P, ctypes.POINTER(RtuDenoiseDesc), _P)


# temporal accumulation (include/rtu_render.h, "Temporal accumulation")
RTU_TEMPORAL_DENOISE = 1


class RtuTemporalDesc(ctypes.Structure):
    """include/rtu_render.h RtuTemporalDesc (32 bytes): the size of the image, the three constants of the accumulator, the session's flags."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("max_history", ctypes.c_int32), ("sigma_plane", ctypes.c_float),
                ("normal_min", ctypes.c_float), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


_sig(hip, "rtu_camera_sample_rays_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _I, _P, _P, _P)
_sig(hip, "rtu_temporal_defaults", _I, ctypes.POINTER(RtuTemporalDesc))
_sig(hip, "rtu_temporal_accumulate", _I, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc), _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_accumulate_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc),
     _P, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_begin", _P, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(_I))
_sig(hip, "rtu_temporal_frame_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _P)
_sig(hip, "rtu_temporal_frame", _I, _P, ctypes.POINTER(RtuFrameDesc), _P)
_sig(hip, "rtu_temporal_history_device", _I, _P, _P, _P)
_sig(hip, "rtu_temporal_reset", _I, _P)
_sig(hip, "rtu_temporal_free", None, _P)


def temporal_desc(width=0, height=0, denoise=False, **overrides):
    """An RtuTemporalDesc: rtu_temporal_defaults (max_history 32, sigma_plane 0.05, normal_min 0.9), the size, RTU_TEMPORAL_DENOISE
    for denoise=True (read by sessions only), then `overrides`."""
    d = RtuTemporalDesc()
    hip.rtu_temporal_defaults(ctypes.byref(d))
    d.width, d.height = int(width), int(height)
    d.flags = RTU_TEMPORAL_DENOISE if denoise else 0
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


def _temporal_accumulate(planes, call, prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc, motion=None, history_cap=0):
    """What the three temporal_accumulate*() share: the arrays validated, desc copied and sized from rgbz, `call` (the host form of
    librtu_hip, with a history of `planes` planes; motion None: the form that takes no table) -> (rc, accumulated rgbz, new history)."""
    import numpy as np
    rgbz = np.ascontiguousarray(rgbz, np.float32)
    if rgbz.ndim != 3 or rgbz.shape[2] != 4:
        raise RtuError(RTU_ERR_ARG, "rgbz: a float32 [H, W, 4] array")
    H, W = rgbz.shape[:2]
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]")
    if hist_prev is not None:
        hist_prev = np.ascontiguousarray(hist_prev, np.float32)
        if hist_prev.size != 4 * planes * H * W:
            raise RtuError(RTU_ERR_ARG, "hist_prev: float32 [%d, H, W, 4]" % planes)
    table = ()
    if motion is not None:
        motion = _as_motion(motion)
        table = (motion.ctypes.data if len(motion) else ctypes.addressof(ctypes.c_char()), len(motion), int(history_cap))
    d = RtuTemporalDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else temporal_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    out, hist = np.empty_like(rgbz), np.empty((planes, H, W, 4), np.float32)
    rc = call(ctypes.byref(d), ctypes.byref(prev_cam) if prev_cam is not None else None, ctypes.byref(cur_cam), rgbz.ctypes.data, hits.ctypes.data,
              albedo.ctypes.data, hist_prev.ctypes.data if hist_prev is not None else None, hist.ctypes.data, out.ctypes.data, *table)
    return rc, out, hist


def temporal_accumulate(prev_cam, cur_cam, rgbz, hits, albedo, hist_prev=None, desc=None):
    """rtu_temporal_accumulate (pure host code, the specification of the accumulator): one new sample rgbz float32 [H, W, 4] with the
    guides hits [H * W] of hit_dtype() and albedo float32 [H * W, 4] of cur_cam (an RtuFrameDesc) blended into hist_prev — float32
    [3, H, W, 4], the planes E, P, N of the frame before, whose camera was prev_cam; None: no history — -> (accumulated rgbz
    [H, W, 4], the new history [3, H, W, 4]). desc: an RtuTemporalDesc whose width and height are taken from rgbz (None: the defaults)."""
    rc, out, hist = _temporal_accumulate(3, hip.rtu_temporal_accumulate, prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_accumulate: a descriptor outside its rules (max_history 1..65535, sigma_plane > 0, normal_min "
                           "-1..1, known flags, reserved words 0) or a camera of another size")
    return out, hist


# temporal accumulation across scene updates (include/rtu_render.h): the per-node motion table
RTU_MOTION_STATIC, RTU_MOTION_RESET = 1, 2
RTU_MOTION_DEFORM = 4
_U32 = ctypes.c_uint32
_sig(hip, "rtu_scene_motion", _I, _P, _P, _P, _I, _P)
_sig(hip, "rtu_temporal_accumulate_motion", _I, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc),
     _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32)
_sig(hip, "rtu_temporal_accumulate_motion_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc),
     _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32, _P)
_sig(hip, "rtu_motion_vectors", _I, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), _P, _P, _U32, _P)
_sig(hip, "rtu_motion_vectors_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), _P, _P, _U32, _P, _P)
_sig(hip, "rtu_temporal_frame_moved_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _U32, ctypes.c_int32, _P, _P)
_sig(hip, "rtu_temporal_frame_moved", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _U32, ctypes.c_int32, _P)
# deforming meshes (include/rtu_render.h, "Temporal accumulation on deforming meshes")
_sig(hip, "rtu_keep_previous_vertices", _I, _P, _I)
_sig(hip, "rtu_scene_motion_deform", _I, _P, _P, _P, _I, _P, _I, _P)
for _name in ("rtu_temporal_accumulate_deform", "rtu_temporal_accumulate_deform_moments"):
    _sig(hip, _name, _I, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc),
         _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32)
    _sig(hip, _name + "_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc),
         _P, _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32, _P)
_sig(hip, "rtu_temporal_frame_deformed_device", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _U32, ctypes.c_int32, _P, _P)
_sig(hip, "rtu_temporal_frame_deformed", _I, _P, ctypes.POINTER(RtuFrameDesc), _P, _U32, ctypes.c_int32, _P)
_sig(hip, "rtu_motion_vectors_deform", _I, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), _P, _P, _P, _P, _U32, _P)
_sig(hip, "rtu_motion_vectors_deform_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), _P, _P, _P, _U32, _P, _P)


def motion_dtype():
    """RtuNodeMotion (96 bytes) as a numpy structured dtype: m [3, 4] (prev_from_cur, rows {a, b, c, d}), g [3, 3], flags, reserved."""
    import numpy as np
    return np.dtype([("m", np.float32, (3, 4)), ("g", np.float32, (3, 3)), ("flags", np.uint32), ("reserved", np.uint32, (2,))])


def _as_motion(motion):
    import numpy as np
    motion = np.ascontiguousarray(motion)
    if motion.dtype != motion_dtype() or motion.ndim != 1:
        raise RtuError(RTU_ERR_ARG, "motion: a 1-d array of motion_dtype()")
    return motion


def scene_motion(prev, cur, reset_meshes=(), deform_meshes=None):
    """rtu_scene_motion (pure host code): for every node of the Scene `cur` the affine map that carries a point of that node's surface
    to where it was in the Scene `prev` (same shape), as an array of motion_dtype(). Nodes whose chain did not change are
    RTU_MOTION_STATIC; nodes of the meshes in reset_meshes (those given to update_meshes) are RTU_MOTION_RESET. deform_meshes (not
    None: rtu_scene_motion_deform): nodes of those meshes are RTU_MOTION_DEFORM — m is W_prev — for temporal_accumulate_deform()."""
    import numpy as np
    out = np.zeros(cur.desc.n_nodes, motion_dtype())
    ids = (ctypes.c_uint32 * max(1, len(reset_meshes)))(*reset_meshes)
    if deform_meshes is not None:
        dids = (ctypes.c_uint32 * max(1, len(deform_meshes)))(*deform_meshes)
        rc = hip.rtu_scene_motion_deform(prev.desc_ptr, cur.desc_ptr, dids, len(deform_meshes), ids, len(reset_meshes), out.ctypes.data)
    else:
        rc = hip.rtu_scene_motion(prev.desc_ptr, cur.desc_ptr, ids, len(reset_meshes), out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_scene_motion: " + ("a mesh id outside the scene's meshes" if rc == RTU_ERR_ARG else scene_shape_diff(prev, cur) or ""))
    return out


def temporal_accumulate_motion(prev_cam, cur_cam, rgbz, hits, albedo, motion, hist_prev=None, desc=None, history_cap=0):
    """rtu_temporal_accumulate_motion (pure host code): temporal_accumulate() across a scene update — `motion` (motion_dtype(), see
    scene_motion()) carries every pixel's hit point to the previous frame's scene before the lookup; history_cap 0 (none) .. 65535
    bounds the history length a pixel takes over. -> (accumulated rgbz [H, W, 4], the new history [3, H, W, 4])."""
    rc, out, hist = _temporal_accumulate(3, hip.rtu_temporal_accumulate_motion, prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc, motion, history_cap)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_accumulate_motion: a descriptor outside its rules, a camera of another size, history_cap outside "
                           "0..65535, or a table entry with an unknown flag or a non-zero reserved word")
    return out, hist


def _as_surface(surface, n):
    import numpy as np
    surface = np.ascontiguousarray(surface)
    if surface.dtype != surface_dtype() or surface.size != n:
        raise RtuError(RTU_ERR_ARG, "surface: H * W of surface_dtype()")
    return surface


def temporal_accumulate_deform(prev_cam, cur_cam, rgbz, hits, albedo, surface, prev_scene, motion, hist_prev=None, desc=None, history_cap=0,
                               moments=False):
    """rtu_temporal_accumulate_deform / _deform_moments (pure host code): temporal_accumulate_motion() / _moments() that follows
    deforming meshes — where a pixel's table entry is RTU_MOTION_DEFORM (scene_motion(deform_meshes=)), its surface record
    (frame_surface / ray_surface: face and weights) is evaluated over the vertices of the Scene `prev_scene` and carried through the
    entry before the lookup. -> (accumulated rgbz [H, W, 4], the new history [3 or 4, H, W, 4])."""
    import numpy as np
    surface = _as_surface(surface, np.asarray(rgbz).shape[0] * np.asarray(rgbz).shape[1])
    fn = hip.rtu_temporal_accumulate_deform_moments if moments else hip.rtu_temporal_accumulate_deform

    def call(d, pc, cc, r, h, a, hp, ho, o, *table):
        return fn(d, pc, cc, r, h, a, surface.ctypes.data, prev_scene.desc_ptr, hp, ho, o, *table)
    rc, out, hist = _temporal_accumulate(4 if moments else 3, call, prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc, motion, history_cap)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_accumulate_deform: what temporal_accumulate_motion refuses, or a table of another length than "
                           "prev_scene's node count")
    return out, hist


def motion_vectors_deform(prev_cam, hits, surface, prev_scene, motion, width, height):
    """rtu_motion_vectors_deform (pure host code): motion_vectors() with the previous position of RTU_MOTION_DEFORM pixels taken
    from their surface records over the vertices of `prev_scene`."""
    import numpy as np
    hits = np.ascontiguousarray(hits)
    if hits.dtype != hit_dtype() or hits.size != width * height:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype()")
    surface = _as_surface(surface, width * height)
    motion = _as_motion(motion)
    d = temporal_desc(width, height)
    out = np.empty((height, width, 4), np.float32)
    rc = hip.rtu_motion_vectors_deform(ctypes.byref(d), ctypes.byref(prev_cam), hits.ctypes.data, surface.ctypes.data, prev_scene.desc_ptr,
                                       motion.ctypes.data if len(motion) else ctypes.addressof(ctypes.c_char()), len(motion), out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_motion_vectors_deform: what motion_vectors refuses, or a table of another length than prev_scene's node count")
    return out


def motion_vectors(prev_cam, hits, motion, width, height):
    """rtu_motion_vectors (pure host code): float32 [H, W, 4] — per pixel {fx, fy, 1, 0}, the continuous coordinates in the image of
    prev_cam (an integer is a pixel centre) where the pixel's surface point was before the update described by `motion`, or zeros."""
    import numpy as np
    hits = np.ascontiguousarray(hits)
    if hits.dtype != hit_dtype() or hits.size != width * height:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype()")
    motion = _as_motion(motion)
    d = temporal_desc(width, height)
    out = np.empty((height, width, 4), np.float32)
    rc = hip.rtu_motion_vectors(ctypes.byref(d), ctypes.byref(prev_cam), hits.ctypes.data,
                                motion.ctypes.data if len(motion) else ctypes.addressof(ctypes.c_char()), len(motion), out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_motion_vectors: a camera of another size or a table entry with an unknown flag or a non-zero reserved word")
    return out


def denoise_desc(width=0, height=0, **overrides):
    """An RtuDenoiseDesc: rtu_denoise_defaults (n_passes 5, sigma_color 1, sigma_plane 0.05, normal_log2_power 5), the size, then `overrides`."""
    d = RtuDenoiseDesc()
    hip.rtu_denoise_defaults(ctypes.byref(d))
    d.width, d.height = int(width), int(height)
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


def denoise(rgbz, hits, albedo, desc=None):
    """rtu_denoise (pure host code, the specification of the filter): rgbz float32 [H, W, 4], hits [H * W] of hit_dtype() and albedo
    float32 [H * W, 4] as frame_features / ray_features return them -> the filtered float32 [H, W, 4]. desc: an RtuDenoiseDesc whose
    width and height are taken from rgbz (None: the defaults)."""
    import numpy as np
    rgbz = np.ascontiguousarray(rgbz, np.float32)
    if rgbz.ndim != 3 or rgbz.shape[2] != 4:
        raise RtuError(RTU_ERR_ARG, "rgbz: a float32 [H, W, 4] array")
    H, W = rgbz.shape[:2]
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]")
    d = RtuDenoiseDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else denoise_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    out = np.empty_like(rgbz)
    rc = hip.rtu_denoise(ctypes.byref(d), rgbz.ctypes.data, hits.ctypes.data, albedo.ctypes.data, out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_denoise: an empty image or a descriptor outside its rules (n_passes 1..8, sigmas > 0, "
                           "normal_log2_power 0..7, reserved words 0)")
    return out


# variance-guided filtering (include/rtu_render.h, "Variance-guided filtering")
class RtuVarianceDesc(ctypes.Structure):
    """include/rtu_render.h RtuVarianceDesc (40 bytes): the size of the image, the constants of the variance and of its filter."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("n_passes", ctypes.c_int32), ("sigma_lum", ctypes.c_float),
                ("sigma_plane", ctypes.c_float), ("normal_log2_power", ctypes.c_int32), ("min_history", ctypes.c_int32),
                ("reserved", ctypes.c_uint32 * 3)]


_sig(hip, "rtu_variance_defaults", _I, ctypes.POINTER(RtuVarianceDesc))
_sig(hip, "rtu_temporal_accumulate_moments", _I, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc),
     _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32)
_sig(hip, "rtu_temporal_accumulate_moments_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuFrameDesc), ctypes.POINTER(RtuFrameDesc),
     _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32, _P)
_sig(hip, "rtu_variance", _I, ctypes.POINTER(RtuVarianceDesc), _P, _P, _P)
_sig(hip, "rtu_variance_device", _I, _P, ctypes.POINTER(RtuVarianceDesc), _P, _P, _P, _P)
_sig(hip, "rtu_denoise_variance", _I, ctypes.POINTER(RtuVarianceDesc), _P, _P, _P, _P, _P)
_sig(hip, "rtu_denoise_variance_device", _I, _P, ctypes.POINTER(RtuVarianceDesc), _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_begin_variance", _P, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuVarianceDesc), ctypes.POINTER(_I))


def variance_desc(width=0, height=0, **overrides):
    """An RtuVarianceDesc: rtu_variance_defaults (n_passes 3, sigma_lum 2, sigma_plane 0.05, normal_log2_power 5, min_history 4), the
    size, then `overrides`."""
    d = RtuVarianceDesc()
    hip.rtu_variance_defaults(ctypes.byref(d))
    d.width, d.height = int(width), int(height)
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


def _sized_variance_desc(desc, W, H):
    d = RtuVarianceDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else variance_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    return d


def temporal_accumulate_moments(prev_cam, cur_cam, rgbz, hits, albedo, motion, hist_prev=None, desc=None, history_cap=0):
    """rtu_temporal_accumulate_moments (pure host code): temporal_accumulate_motion() on a moments history, float32 [4, H, W, 4] — the
    planes E, P, N and M = {m1, m2, 0, 0}, the running moments of the sample's luminance. -> (accumulated rgbz [H, W, 4], the new
    history [4, H, W, 4]); the image and the first three planes are temporal_accumulate_motion()'s bits."""
    rc, out, hist = _temporal_accumulate(4, hip.rtu_temporal_accumulate_moments, prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc, motion, history_cap)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_accumulate_moments: a descriptor outside its rules, a camera of another size, history_cap outside "
                           "0..65535, or a table entry with an unknown flag or a non-zero reserved word")
    return out, hist


def variance(hist, hits, desc=None):
    """rtu_variance (pure host code): the variance of the accumulated mean's luminance per pixel, float32 [H, W], out of a moments
    history float32 [4, H, W, 4] and the hits [H * W] of its frame; 0 for a pixel without history. desc: an RtuVarianceDesc whose
    width and height are taken from hist (None: the defaults)."""
    import numpy as np
    hist = np.ascontiguousarray(hist, np.float32)
    if hist.ndim != 4 or hist.shape[0] != 4 or hist.shape[3] != 4:
        raise RtuError(RTU_ERR_ARG, "hist: a float32 [4, H, W, 4] array")
    H, W = hist.shape[1:3]
    hits = np.ascontiguousarray(hits)
    if hits.dtype != hit_dtype() or hits.size != H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype()")
    d = _sized_variance_desc(desc, W, H)
    out = np.empty((H, W), np.float32)
    rc = hip.rtu_variance(ctypes.byref(d), hist.ctypes.data, hits.ctypes.data, out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_variance: an empty image or a descriptor outside its rules (n_passes 1..8, sigmas > 0, normal_log2_power "
                           "0..7, min_history 1..65535, reserved words 0)")
    return out


def denoise_variance(rgbz, hits, albedo, v, desc=None):
    """rtu_denoise_variance (pure host code, the specification of the filter): denoise() with a colour edge-stop per pixel, set by the
    variance v float32 [H, W] (see variance()) -> the filtered float32 [H, W, 4]."""
    import numpy as np
    rgbz = np.ascontiguousarray(rgbz, np.float32)
    if rgbz.ndim != 3 or rgbz.shape[2] != 4:
        raise RtuError(RTU_ERR_ARG, "rgbz: a float32 [H, W, 4] array")
    H, W = rgbz.shape[:2]
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    v = np.ascontiguousarray(v, np.float32)
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W or v.size != H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]; v: float32 [H, W]")
    d = _sized_variance_desc(desc, W, H)
    out = np.empty_like(rgbz)
    rc = hip.rtu_denoise_variance(ctypes.byref(d), rgbz.ctypes.data, hits.ctypes.data, albedo.ctypes.data, v.ctypes.data, out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_denoise_variance: an empty image or a descriptor outside its rules (n_passes 1..8, sigmas > 0, "
                           "normal_log2_power 0..7, min_history 1..65535, reserved words 0)")
    return out


# steered sampling (include/rtu_render.h, "Steered sampling")
class RtuSteerDesc(ctypes.Structure):
    """include/rtu_render.h RtuSteerDesc (32 bytes): the size of the image, the budget of extra rays of a frame, the most a pixel gets,
    and the frame's index."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("budget", ctypes.c_uint32), ("max_extra", ctypes.c_int32),
                ("frame_index", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


_sig(hip, "rtu_steer_defaults", _I, ctypes.POINTER(RtuSteerDesc))
_sig(hip, "rtu_sample_allocation", _I, ctypes.POINTER(RtuSteerDesc), _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_sample_allocation_device", _I, _P, ctypes.POINTER(RtuSteerDesc), _P, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_extra_sample_rays", _I, ctypes.POINTER(RtuSteerDesc), ctypes.POINTER(RtuFrameDesc), _P, _P, ctypes.c_size_t, _P, _P, _P)
_sig(hip, "rtu_extra_sample_rays_device", _I, _P, ctypes.POINTER(RtuSteerDesc), ctypes.POINTER(RtuFrameDesc), _P, _P, ctypes.c_size_t, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_refine", _I, ctypes.POINTER(RtuTemporalDesc), _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P)
_sig(hip, "rtu_temporal_refine_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P, _P)
_sig(hip, "rtu_temporal_begin_steered", _P, _P, ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuVarianceDesc), ctypes.POINTER(RtuSteerDesc),
     ctypes.POINTER(_I))
_sig(hip, "rtu_temporal_extra_counts_device", _I, _P, _P, _P)
_sig(hip, "rtu_temporal_steer_total", _I, _P, ctypes.POINTER(_U32))


def steer_desc(width=0, height=0, **overrides):
    """An RtuSteerDesc: rtu_steer_defaults (budget 0, max_extra 3, frame_index 0), the size, then `overrides`."""
    d = RtuSteerDesc()
    hip.rtu_steer_defaults(ctypes.byref(d))
    d.width, d.height = int(width), int(height)
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


def _sized_steer_desc(desc, W, H):
    d = RtuSteerDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else steer_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    return d


def sample_allocation(hist, hits, v, desc):
    """rtu_sample_allocation (pure host code): desc.budget extra rays spread over the pixels by the variance v float32 [H, W] of the
    moments history float32 [4, H, W, 4] (see variance()), at most desc.max_extra each -> (counts uint32 [H, W], offsets uint32
    [H, W], total). The width and height of desc are taken from hist."""
    import numpy as np
    hist = np.ascontiguousarray(hist, np.float32)
    if hist.ndim != 4 or hist.shape[0] != 4 or hist.shape[3] != 4:
        raise RtuError(RTU_ERR_ARG, "hist: a float32 [4, H, W, 4] array")
    H, W = hist.shape[1:3]
    hits = np.ascontiguousarray(hits)
    v = np.ascontiguousarray(v, np.float32)
    if hits.dtype != hit_dtype() or hits.size != H * W or v.size != H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); v: float32 [H, W]")
    d = _sized_steer_desc(desc, W, H)
    counts, offsets, total = np.empty((H, W), np.uint32), np.empty((H, W), np.uint32), _U32(0)
    rc = hip.rtu_sample_allocation(ctypes.byref(d), hist.ctypes.data, hits.ctypes.data, v.ctypes.data, counts.ctypes.data, offsets.ctypes.data,
                                   ctypes.byref(total))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_sample_allocation: an empty image or a descriptor outside its rules (budget 0..2^26, max_extra 1..15, "
                           "reserved words 0)")
    return counts, offsets, int(total.value)


def extra_sample_rays(frame, counts, offsets, desc, capacity=None):
    """rtu_extra_sample_rays (pure host code): the extra rays of frame desc.frame_index of the recipe S / P frame `frame` for the
    counts and offsets of sample_allocation() -> (rays [capacity] of ray_dtype(), keys uint32, owner uint32). capacity: None is the
    number of rays the counts and offsets name."""
    import numpy as np
    counts = np.ascontiguousarray(counts, np.uint32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    if counts.size != frame.width * frame.height or offsets.size != counts.size:
        raise RtuError(RTU_ERR_ARG, "counts, offsets: uint32 [H, W] of the frame")
    if capacity is None:
        capacity = int((offsets.astype(np.uint64) + counts).max()) if counts.size and counts.any() else 0
    d = _sized_steer_desc(desc, frame.width, frame.height)
    rays, keys, owner = np.zeros(capacity, ray_dtype()), np.zeros(capacity, np.uint32), np.zeros(capacity, np.uint32)
    rc = hip.rtu_extra_sample_rays(ctypes.byref(d), ctypes.byref(frame), counts.ctypes.data, offsets.ctypes.data, capacity,
                                   rays.ctypes.data if capacity else None, keys.ctypes.data if capacity else None,
                                   owner.ctypes.data if capacity else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_extra_sample_rays: a descriptor outside its rules, not a recipe S frame, samples * (1 + max_extra) > 65536, "
                           "a count above max_extra or a ray beyond the capacity")
    return rays, keys, owner


def temporal_refine(hist, rgbz, hits, albedo, counts, offsets, rgbt, desc=None):
    """rtu_temporal_refine (pure host code): the shaded extra samples rgbt float32 [n, 4] folded into the moments history float32
    [4, H, W, 4] and the image rgbz [H, W, 4] -> (rgbz, hist), new arrays (the C entry works in place). Of desc (an RtuTemporalDesc,
    None: the defaults) max_history is used."""
    import numpy as np
    hist = np.array(hist, np.float32, order="C")
    rgbz = np.array(rgbz, np.float32, order="C")
    if hist.ndim != 4 or hist.shape[0] != 4 or hist.shape[3] != 4 or rgbz.shape != hist.shape[1:]:
        raise RtuError(RTU_ERR_ARG, "hist: a float32 [4, H, W, 4] array; rgbz: float32 [H, W, 4]")
    H, W = hist.shape[1:3]
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    counts = np.ascontiguousarray(counts, np.uint32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    rgbt = np.ascontiguousarray(rgbt, np.float32).reshape(-1, 4)
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W or counts.size != H * W or offsets.size != H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]; counts, offsets: uint32 [H, W]")
    d = RtuTemporalDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else temporal_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    rc = hip.rtu_temporal_refine(ctypes.byref(d), hist.ctypes.data, hits.ctypes.data, albedo.ctypes.data, counts.ctypes.data, offsets.ctypes.data,
                                 rgbt.ctypes.data if len(rgbt) else None, len(rgbt), rgbz.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_refine: a descriptor outside its rules, or a pixel whose samples lie beyond rgbt")
    return rgbz, hist


# temporal gradients (include/rtu_render.h, "Temporal gradients")
class RtuGradientDesc(ctypes.Structure):
    """include/rtu_render.h RtuGradientDesc (32 bytes): the size of the image, the radius (in strata) lambda is summed over, the noise
    floor kappa, the session's switch and the frame's index."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("radius", ctypes.c_int32), ("kappa", ctypes.c_float),
                ("enabled", ctypes.c_uint32), ("frame_index", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


_TD, _GD, _FD = ctypes.POINTER(RtuTemporalDesc), ctypes.POINTER(RtuGradientDesc), ctypes.POINTER(RtuFrameDesc)
_sig(hip, "rtu_gradient_defaults", _I, _GD)
_sig(hip, "rtu_gradient_rays", _I, _GD, _FD, _I, _P, _P, _P)
_sig(hip, "rtu_gradient_rays_device", _I, _P, _GD, _FD, _I, _P, _P, _P, _P)
_sig(hip, "rtu_sample_luminance", _I, _GD, _P, _P, _P, _P)
_sig(hip, "rtu_sample_luminance_device", _I, _P, _GD, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_gradient", _I, _TD, _GD, _FD, _FD, _P, _P, _P, _U32, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_gradient_device", _I, _P, _TD, _GD, _FD, _FD, _P, _P, _P, _U32, _P, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_accumulate_gradient", _I, _TD, _FD, _FD, _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32, _P)
_sig(hip, "rtu_temporal_accumulate_gradient_device", _I, _P, _TD, _FD, _FD, _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32, _P, _P)
_sig(hip, "rtu_temporal_begin_gradient", _P, _P, _TD, ctypes.POINTER(RtuVarianceDesc), ctypes.POINTER(RtuSteerDesc), _GD, ctypes.POINTER(_I))
_sig(hip, "rtu_temporal_lambda_device", _I, _P, _P, _P)


def gradient_desc(width=0, height=0, **overrides):
    """An RtuGradientDesc: rtu_gradient_defaults (radius 1, kappa 2, enabled 1, frame_index 0), the size, then `overrides`."""
    d = RtuGradientDesc()
    hip.rtu_gradient_defaults(ctypes.byref(d))
    d.width, d.height = int(width), int(height)
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


def _sized_gradient_desc(desc, W, H):
    d = RtuGradientDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else gradient_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    return d


def strata(width, height):
    """(SW, SH): the 3 x 3 strata of a width x height image."""
    return (width + 2) // 3, (height + 2) // 3


def gradient_rays(frame, sample, desc=None):
    """rtu_gradient_rays (pure host code): per stratum the pixel it owns in frame desc.frame_index and that pixel's ray and key of
    camera_sample_rays(frame, sample) -> (rays [SW * SH] of ray_dtype(), keys uint32, owner uint32)."""
    import numpy as np
    d = _sized_gradient_desc(desc, frame.width, frame.height)
    sw, sh = strata(frame.width, frame.height)
    rays, keys, owner = np.zeros(sw * sh, ray_dtype()), np.zeros(sw * sh, np.uint32), np.zeros(sw * sh, np.uint32)
    rc = hip.rtu_gradient_rays(ctypes.byref(d), ctypes.byref(frame), int(sample), rays.ctypes.data, keys.ctypes.data, owner.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_gradient_rays: a descriptor outside its rules (radius 0..3, kappa >= 0, enabled 0 or 1, reserved words 0), "
                           "not a recipe S frame or a sample outside [0, samples)")
    return rays, keys, owner


def sample_luminance(rgbz, hits, albedo):
    """rtu_sample_luminance (pure host code): float32 [H, W], the luminance of the demodulated raw sample rgbz float32 [H, W, 4]; 0 for
    a pixel that is not valid or not finite."""
    import numpy as np
    rgbz = np.ascontiguousarray(rgbz, np.float32)
    if rgbz.ndim != 3 or rgbz.shape[2] != 4:
        raise RtuError(RTU_ERR_ARG, "rgbz: a float32 [H, W, 4] array")
    H, W = rgbz.shape[:2]
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]")
    d = gradient_desc(W, H)
    out = np.empty((H, W), np.float32)
    rc = hip.rtu_sample_luminance(ctypes.byref(d), rgbz.ctypes.data, hits.ctypes.data, albedo.ctypes.data, out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_sample_luminance: an empty image")
    return out


def temporal_gradient(prev_cam, cur_cam, hits, albedo, motion, hist_prev, lum_prev, owner, rgbt, desc=None, gradient=None):
    """rtu_temporal_gradient (pure host code): the gradient rays' shaded samples rgbt float32 [SW * SH, 4] of the owners `owner`
    (see gradient_rays()) against lum_prev float32 [H, W] (sample_luminance() of the previous frame) where the accumulator looks the
    owner's history up in hist_prev float32 [4, H, W, 4] -> (diff float32 [SH, SW, 4] = {num, den, noise, 0}, lambda float32 [SH, SW]).
    hist_prev None: no gradient anywhere. desc: an RtuTemporalDesc, gradient: an RtuGradientDesc, both sized from cur_cam."""
    import numpy as np
    W, H = cur_cam.width, cur_cam.height
    sw, sh = strata(W, H)
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    owner = np.ascontiguousarray(owner, np.uint32)
    rgbt = np.ascontiguousarray(rgbt, np.float32)
    motion = _as_motion(motion)
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W or owner.size != sw * sh or rgbt.size != 4 * sw * sh:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]; owner: uint32 [SW * SH]; rgbt: float32 [SW * SH, 4]")
    if hist_prev is not None:
        hist_prev = np.ascontiguousarray(hist_prev, np.float32)
        lum_prev = np.ascontiguousarray(lum_prev, np.float32)
        if hist_prev.size != 16 * H * W or lum_prev.size != H * W:
            raise RtuError(RTU_ERR_ARG, "hist_prev: float32 [4, H, W, 4]; lum_prev: float32 [H, W]")
    td = RtuTemporalDesc()
    ctypes.memmove(ctypes.byref(td), ctypes.byref(desc if desc is not None else temporal_desc()), ctypes.sizeof(td))
    td.width, td.height = W, H
    gd = _sized_gradient_desc(gradient, W, H)
    diff, lam = np.empty((sh, sw, 4), np.float32), np.empty((sh, sw), np.float32)
    rc = hip.rtu_temporal_gradient(ctypes.byref(td), ctypes.byref(gd), ctypes.byref(prev_cam) if prev_cam is not None else None, ctypes.byref(cur_cam),
                                   hits.ctypes.data, albedo.ctypes.data, motion.ctypes.data if len(motion) else ctypes.addressof(ctypes.c_char()),
                                   len(motion), hist_prev.ctypes.data if hist_prev is not None else None,
                                   lum_prev.ctypes.data if hist_prev is not None else None, owner.ctypes.data, rgbt.ctypes.data, diff.ctypes.data,
                                   lam.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_gradient: a descriptor outside its rules, a camera of another size, an owner outside the image, or a "
                           "table entry with an unknown flag or a non-zero reserved word")
    return diff, lam


def temporal_accumulate_gradient(prev_cam, cur_cam, rgbz, hits, albedo, motion, hist_prev=None, desc=None, history_cap=0, lam=None):
    """rtu_temporal_accumulate_gradient (pure host code): temporal_accumulate_moments() whose history taken over is capped once more,
    per pixel, by lam float32 [SH, SW] (see temporal_gradient(); None: the moments form's bits) -> (accumulated rgbz, new history)."""
    import numpy as np
    if lam is not None:
        H, W = np.shape(rgbz)[:2]
        lam = np.ascontiguousarray(lam, np.float32)
        if lam.size != strata(W, H)[0] * strata(W, H)[1]:
            raise RtuError(RTU_ERR_ARG, "lam: float32 [SH, SW]")
    call = lambda *a: hip.rtu_temporal_accumulate_gradient(*a, lam.ctypes.data if lam is not None else None)
    rc, out, hist = _temporal_accumulate(4, call, prev_cam, cur_cam, rgbz, hits, albedo, hist_prev, desc, motion, history_cap)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_accumulate_gradient: a descriptor outside its rules, a camera of another size, history_cap outside "
                           "0..65535, or a table entry with an unknown flag or a non-zero reserved word")
    return out, hist


# sparse sessions (include/rtu_render.h, "Sparse sessions")
class RtuSparseDesc(ctypes.Structure):
    """include/rtu_render.h RtuSparseDesc (32 bytes): the size of the image, the block size B and the frame's index."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("block", ctypes.c_int32), ("frame_index", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 4)]


_SD = ctypes.POINTER(RtuSparseDesc)
_sig(hip, "rtu_sparse_defaults", _I, _SD)
_sig(hip, "rtu_sparse_rays", _I, _SD, _FD, _P, _P, _P)
_sig(hip, "rtu_sparse_rays_device", _I, _P, _SD, _FD, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_accumulate_sparse", _I, _TD, _SD, _FD, _FD, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32)
_sig(hip, "rtu_temporal_accumulate_sparse_device", _I, _P, _TD, _SD, _FD, _FD, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, ctypes.c_int32, _P)
_sig(hip, "rtu_sparse_fill", _I, _TD, _SD, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_sparse_fill_device", _I, _P, _TD, _SD, _P, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_begin_sparse", _P, _P, _TD, ctypes.POINTER(RtuVarianceDesc), _SD, ctypes.POINTER(_I))
_sig(hip, "rtu_temporal_holes", _I, _P, ctypes.POINTER(_U32))


def sparse_desc(width=0, height=0, **overrides):
    """An RtuSparseDesc: rtu_sparse_defaults (block 2, frame_index 0), the size, then `overrides`."""
    d = RtuSparseDesc()
    hip.rtu_sparse_defaults(ctypes.byref(d))
    d.width, d.height = int(width), int(height)
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


def _sized_sparse_desc(desc, W, H):
    d = RtuSparseDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else sparse_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    return d


def sparse_blocks(width, height, block):
    """(SW, SH): the block x block blocks of a width x height image."""
    return (width + block - 1) // block, (height + block - 1) // block


def sparse_rays(frame, desc=None):
    """rtu_sparse_rays (pure host code): per block the pixel it owns in frame desc.frame_index and that pixel's ray and key in the
    sample the block has reached -> (rays [SW * SH] of ray_dtype(), keys uint32, owner uint32). The size of desc is the frame's."""
    import numpy as np
    d = _sized_sparse_desc(desc, frame.width, frame.height)
    n = 0
    if 1 <= d.block <= 4:
        sw, sh = sparse_blocks(frame.width, frame.height, d.block)
        n = max(sw, 0) * max(sh, 0)
    rays, keys, owner = np.zeros(max(n, 1), ray_dtype()), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    rc = hip.rtu_sparse_rays(ctypes.byref(d), ctypes.byref(frame), rays.ctypes.data, keys.ctypes.data, owner.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_sparse_rays: a descriptor outside its rules (block 1..4, reserved words 0) or not a recipe S frame")
    return rays[:n], keys[:n], owner[:n]


def temporal_accumulate_sparse(prev_cam, cur_cam, rgbt, owner, hits, albedo, motion, hist_prev=None, desc=None, sparse=None, history_cap=0):
    """rtu_temporal_accumulate_sparse (pure host code): temporal_accumulate_moments() whose samples are rgbt float32 [SW * SH, 4], the
    shaded rays of sparse_rays(), at the pixels `owner`; every other pixel keeps its history -> (rgbz [H, W, 4], the new history
    [4, H, W, 4], hole uint8 [H, W]: 1 where a pixel has no colour). desc: an RtuTemporalDesc, sparse: an RtuSparseDesc, both sized
    from cur_cam."""
    import numpy as np
    W, H = cur_cam.width, cur_cam.height
    sd = _sized_sparse_desc(sparse, W, H)
    rgbt = np.ascontiguousarray(rgbt, np.float32)
    owner = np.ascontiguousarray(owner, np.uint32)
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    motion = _as_motion(motion)
    if 1 <= sd.block <= 4:
        sw, sh = sparse_blocks(W, H, sd.block)
        if owner.size != sw * sh or rgbt.size != 4 * sw * sh:
            raise RtuError(RTU_ERR_ARG, "owner: uint32 [SW * SH]; rgbt: float32 [SW * SH, 4]")
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]")
    if hist_prev is not None:
        hist_prev = np.ascontiguousarray(hist_prev, np.float32)
        if hist_prev.size != 16 * H * W:
            raise RtuError(RTU_ERR_ARG, "hist_prev: float32 [4, H, W, 4]")
    td = RtuTemporalDesc()
    ctypes.memmove(ctypes.byref(td), ctypes.byref(desc if desc is not None else temporal_desc()), ctypes.sizeof(td))
    td.width, td.height = W, H
    out, hist, hole = np.empty((H, W, 4), np.float32), np.empty((4, H, W, 4), np.float32), np.empty((H, W), np.uint8)
    rc = hip.rtu_temporal_accumulate_sparse(ctypes.byref(td), ctypes.byref(sd), ctypes.byref(prev_cam) if prev_cam is not None else None,
                                            ctypes.byref(cur_cam), rgbt.ctypes.data, owner.ctypes.data, hits.ctypes.data, albedo.ctypes.data,
                                            hist_prev.ctypes.data if hist_prev is not None else None, hist.ctypes.data, out.ctypes.data,
                                            hole.ctypes.data, motion.ctypes.data if len(motion) else ctypes.addressof(ctypes.c_char()), len(motion),
                                            int(history_cap))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_accumulate_sparse: a descriptor outside its rules (block 1..4, reserved words 0; see "
                           "temporal_accumulate_moments), a camera of another size, history_cap outside 0..65535, or a table entry with an "
                           "unknown flag or a non-zero reserved word")
    return out, hist, hole


def sparse_fill(rgbz, hole, hits, albedo, owner, rgbt, desc=None, sparse=None):
    """rtu_sparse_fill (pure host code): the pixels of rgbz float32 [H, W, 4] with hole [H, W] == 1 filled from the samples rgbt of the
    neighbouring blocks' owners -> rgbz, a new array (the C entry works in place). Of desc (an RtuTemporalDesc) sigma_plane and
    normal_min are used; sparse: an RtuSparseDesc; both sized from rgbz."""
    import numpy as np
    rgbz = np.array(rgbz, np.float32, order="C")
    if rgbz.ndim != 3 or rgbz.shape[2] != 4:
        raise RtuError(RTU_ERR_ARG, "rgbz: a float32 [H, W, 4] array")
    H, W = rgbz.shape[:2]
    sd = _sized_sparse_desc(sparse, W, H)
    hole = np.ascontiguousarray(hole, np.uint8)
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    rgbt = np.ascontiguousarray(rgbt, np.float32)
    owner = np.ascontiguousarray(owner, np.uint32)
    if 1 <= sd.block <= 4:
        sw, sh = sparse_blocks(W, H, sd.block)
        if owner.size != sw * sh or rgbt.size != 4 * sw * sh:
            raise RtuError(RTU_ERR_ARG, "owner: uint32 [SW * SH]; rgbt: float32 [SW * SH, 4]")
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W or hole.size != H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]; hole: uint8 [H, W]")
    td = RtuTemporalDesc()
    ctypes.memmove(ctypes.byref(td), ctypes.byref(desc if desc is not None else temporal_desc()), ctypes.sizeof(td))
    td.width, td.height = W, H
    rc = hip.rtu_sparse_fill(ctypes.byref(td), ctypes.byref(sd), hits.ctypes.data, albedo.ctypes.data, owner.ctypes.data, rgbt.ctypes.data,
                             hole.ctypes.data, rgbz.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_sparse_fill: a descriptor outside its rules or an owner outside the image")
    return rgbz


# hole rays (include/rtu_render.h, "Hole rays")
class RtuHoleDesc(ctypes.Structure):
    """include/rtu_render.h RtuHoleDesc (32 bytes): the size of the image, the budget of hole rays of a frame and the frame's index."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("budget", ctypes.c_uint32), ("frame_index", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 4)]


_HD = ctypes.POINTER(RtuHoleDesc)
_sig(hip, "rtu_hole_defaults", _I, _HD)
_sig(hip, "rtu_hole_allocation", _I, _HD, _P, _P, _P, _P, _P)
_sig(hip, "rtu_hole_allocation_device", _I, _P, _HD, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_hole_fold", _I, _HD, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t)
_sig(hip, "rtu_hole_fold_device", _I, _P, _HD, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P)
_sig(hip, "rtu_temporal_begin_sparse_holes", _P, _P, _TD, ctypes.POINTER(RtuVarianceDesc), _SD, _HD, ctypes.POINTER(_I))
_sig(hip, "rtu_temporal_hole_rays", _I, _P, ctypes.POINTER(_U32))


def hole_desc(width=0, height=0, **overrides):
    """An RtuHoleDesc: rtu_hole_defaults (budget 0, frame_index 0), the size, then `overrides`."""
    d = RtuHoleDesc()
    hip.rtu_hole_defaults(ctypes.byref(d))
    d.width, d.height = int(width), int(height)
    for k, v in overrides.items():
        setattr(d, k, v)
    return d


def _sized_hole_desc(desc, W, H):
    d = RtuHoleDesc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc if desc is not None else hole_desc()), ctypes.sizeof(d))
    d.width, d.height = W, H
    return d


def hole_allocation(hole, hits, desc):
    """rtu_hole_allocation (pure host code): at most desc.budget rays, one each, for the pixels of hole uint8 [H, W] (the hole plane
    of temporal_accumulate_sparse()) that are 1 and have a first hit in `hits` -> (counts uint32 [H, W], offsets uint32 [H, W],
    total). The width and height of desc are taken from hole."""
    import numpy as np
    hole = np.ascontiguousarray(hole, np.uint8)
    if hole.ndim != 2:
        raise RtuError(RTU_ERR_ARG, "hole: a uint8 [H, W] array")
    H, W = hole.shape
    hits = np.ascontiguousarray(hits)
    if hits.dtype != hit_dtype() or hits.size != H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype()")
    d = _sized_hole_desc(desc, W, H)
    counts, offsets, total = np.empty((H, W), np.uint32), np.empty((H, W), np.uint32), _U32(0)
    rc = hip.rtu_hole_allocation(ctypes.byref(d), hole.ctypes.data, hits.ctypes.data, counts.ctypes.data, offsets.ctypes.data, ctypes.byref(total))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_hole_allocation: an empty image or a descriptor outside its rules (budget 0..2^26, reserved words 0)")
    return counts, offsets, int(total.value)


def hole_fold(hist, rgbz, hole, hits, albedo, counts, offsets, rgbt, desc=None):
    """rtu_hole_fold (pure host code): the shaded hole rays rgbt float32 [n, 4] made the history of their pixels in the moments
    history float32 [4, H, W, 4], the image rgbz [H, W, 4] and the hole plane uint8 [H, W] -> (rgbz, hist, hole), new arrays (the C
    entry works in place). desc: an RtuHoleDesc (None: the defaults), sized from hist."""
    import numpy as np
    hist = np.array(hist, np.float32, order="C")
    rgbz = np.array(rgbz, np.float32, order="C")
    hole = np.array(hole, np.uint8, order="C")
    if hist.ndim != 4 or hist.shape[0] != 4 or hist.shape[3] != 4 or rgbz.shape != hist.shape[1:] or hole.shape != hist.shape[1:3]:
        raise RtuError(RTU_ERR_ARG, "hist: a float32 [4, H, W, 4] array; rgbz: float32 [H, W, 4]; hole: uint8 [H, W]")
    H, W = hist.shape[1:3]
    hits = np.ascontiguousarray(hits)
    albedo = np.ascontiguousarray(albedo, np.float32)
    counts = np.ascontiguousarray(counts, np.uint32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    rgbt = np.ascontiguousarray(rgbt, np.float32).reshape(-1, 4)
    if hits.dtype != hit_dtype() or hits.size != H * W or albedo.size != 4 * H * W or counts.size != H * W or offsets.size != H * W:
        raise RtuError(RTU_ERR_ARG, "hits: H * W of hit_dtype(); albedo: float32 [H * W, 4]; counts, offsets: uint32 [H, W]")
    d = _sized_hole_desc(desc, W, H)
    rc = hip.rtu_hole_fold(ctypes.byref(d), hist.ctypes.data, rgbz.ctypes.data, hole.ctypes.data, hits.ctypes.data, albedo.ctypes.data,
                           counts.ctypes.data, offsets.ctypes.data, rgbt.ctypes.data if len(rgbt) else None, len(rgbt))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_hole_fold: a descriptor outside its rules, a count above 1, or a pixel whose sample lies beyond rgbt")
    return rgbz, hist, hole


def sensor_desc(model, width, height, pos, right, up, forward, samples=0, gather_bounces=0, max_bounce=5, fov_deg=180.0, extent=(1, 1),
                reference_walk=False):
    """An RtuSensorDesc: rtu_sensor_defaults, then the fields. model: RTU_SENSOR_* or "equirect" / "fisheye" / "ortho"; right, up and
    forward are an orthonormal frame, used as given; samples / gather_bounces select the recipe as for frame_setup."""
    d = RtuSensorDesc()
    hip.rtu_sensor_defaults(ctypes.byref(d))
    d.model = SENSOR_MODELS[model] if isinstance(model, str) else int(model)
    d.width, d.height = int(width), int(height)
    d.samples, d.gather_bounces, d.max_bounce = int(samples), int(gather_bounces), int(max_bounce)
    d.flags = RTU_QUERY_REFERENCE_WALK if reference_walk else 0
    d.pos[:] = [float(x) for x in pos]
    d.right[:] = [float(x) for x in right]
    d.up[:] = [float(x) for x in up]
    d.forward[:] = [float(x) for x in forward]
    d.fov_deg = float(fov_deg)
    d.extent[:] = [float(x) for x in extent]
    return d


def sensor_rays(desc, sample=0, row0=0, nrows=None):
    """rtu_sensor_rays (pure host code, the specification of a sensor's rays): the rays and keys of sample `sample` of the sensor, image
    rows [row0, row0 + nrows): (rays [nrows * width] of ray_dtype(), keys uint32 [nrows * width]) in image order. A fisheye sample
    outside the image circle has dir = 0: an invalid ray, which no entry traces."""
    import numpy as np
    if nrows is None:
        nrows = desc.height - row0
    n = max(nrows, 0) * max(desc.width, 0)
    rays, keys = np.zeros(n, ray_dtype()), np.zeros(n, np.uint32)
    rc = hip.rtu_sensor_rays(ctypes.byref(desc), sample, row0, nrows, rays.ctypes.data if n else None, keys.ctypes.data if n else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_sensor_rays: a sensor descriptor out of its rules, sample outside the samples or rows outside the image")
    return rays, keys


# temporal accumulation for sensors (include/rtu_render.h, "Temporal accumulation for sensors")
_SD = ctypes.POINTER(RtuSensorDesc)
_sig(hip, "rtu_sensor_project", _I, _SD, _P, ctypes.c_size_t, _P, _P)
_sig(hip, "rtu_temporal_accumulate_sensor", _I, ctypes.POINTER(RtuTemporalDesc), _SD, _SD, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_accumulate_sensor_moments", _I, ctypes.POINTER(RtuTemporalDesc), _SD, _SD, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_accumulate_sensor_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), _SD, _SD, _P, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_accumulate_sensor_moments_device", _I, _P, ctypes.POINTER(RtuTemporalDesc), _SD, _SD, _P, _P, _P, _P, _P, _P, _P)
_sig(hip, "rtu_temporal_sensor_frame_device", _I, _P, _SD, _P, _P)
_sig(hip, "rtu_temporal_sensor_frame", _I, _P, _SD, _P)


def sensor_project(desc, points):
    """rtu_sensor_project (pure host code, the specification of a sensor's projection): the image coordinates of world points float32
    [n, 3] in sensor `desc` -> (fxfy float32 [n, 2], ok bool [n]); pixel (x, y) has its centre at (x, y), a point without an image
    (behind an orthographic sensor, outside a fisheye's field, at a panorama's pole) has ok False and (0, 0)."""
    import numpy as np
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    fxfy, ok = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    rc = hip.rtu_sensor_project(ctypes.byref(desc), points.ctypes.data if n else None, n, fxfy.ctypes.data if n else None, ok.ctypes.data if n else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_sensor_project: a sensor descriptor out of its rules")
    return fxfy, ok.astype(bool)


def temporal_accumulate_sensor(prev, cur, rgbz, hits, albedo, hist_prev=None, desc=None, moments=False):
    """rtu_temporal_accumulate_sensor / _sensor_moments (pure host code): temporal_accumulate() with RtuSensorDesc prev and cur in place
    of the cameras; the lookup goes through sensor_project() of prev, and an equirectangular sensor's columns wrap. moments: the
    histories are float32 [4, H, W, 4] as for temporal_accumulate_moments(), without a motion table (the scene is at rest).
    -> (accumulated rgbz [H, W, 4], the new history)."""
    call = hip.rtu_temporal_accumulate_sensor_moments if moments else hip.rtu_temporal_accumulate_sensor
    rc, out, hist = _temporal_accumulate(4 if moments else 3, call, prev, cur, rgbz, hits, albedo, hist_prev, desc)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_temporal_accumulate_sensor: a descriptor outside its rules, a sensor outside its rules or of another size, "
                           "or a history without its sensor")
    return out, hist


def shade_desc(eye=(0.0, 0.0, 0.0), max_bounce=5, reference_walk=False):
    """An RtuShadeDesc: rtu_shade_defaults, then the eye, the depth and the counting variant's flag."""
    d = RtuShadeDesc()
    hip.rtu_shade_defaults(ctypes.byref(d))
    d.eye[:] = [float(x) for x in eye]
    d.max_bounce = max_bounce
    d.flags = RTU_QUERY_REFERENCE_WALK if reference_walk else 0
    return d


def ray_dtype():
    """numpy layout of RtuRay (32 bytes): org[3], tmax, dir[3], reserved."""
    import numpy as np
    return np.dtype([("org", np.float32, 3), ("tmax", np.float32), ("dir", np.float32, 3), ("reserved", np.uint32)])


def hit_dtype():
    """numpy layout of RtuRayHit (48 bytes): t, node, flags, material, p[3], pad0, N[3], pad1."""
    import numpy as np
    return np.dtype([("t", np.float32), ("node", np.int32), ("flags", np.uint32), ("material", np.int32),
                     ("p", np.float32, 3), ("pad0", np.float32), ("N", np.float32, 3), ("pad1", np.float32)])


def surface_dtype():
    """numpy layout of RtuRaySurface (32 bytes): mesh, face, bc[3], uvw[3]."""
    import numpy as np
    return np.dtype([("mesh", np.int32), ("face", np.int32), ("bc", np.float32, 3), ("uvw", np.float32, 3)])


def _as_rays(rays):
    """A contiguous RtuRay array from a structured array of ray_dtype() or a float32 [n, 8] array {org, tmax, dir, reserved}."""
    import numpy as np
    rays = np.asarray(rays)
    if rays.dtype == ray_dtype():
        return np.ascontiguousarray(rays).reshape(-1)
    if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8:
        raise RtuError(RTU_ERR_ARG, "rays: a float32 [n, 8] array or a structured array of ray_dtype()")
    return np.ascontiguousarray(rays).view(ray_dtype()).reshape(-1)


def camera_rays(frame, row0=0, nrows=None):
    """rtu_camera_rays (pure host code): the pixel-centre rays of image rows [row0, row0 + nrows) of `frame` as a structured array
    [nrows * width] of ray_dtype(), in image order, tmax = RTU_BIGFLOAT: the primary rays of a render of that frame, bit for bit."""
    import numpy as np
    if nrows is None:
        nrows = frame.height - row0
    out = np.zeros(max(nrows, 0) * max(frame.width, 0), ray_dtype())
    rc = hip.rtu_camera_rays(ctypes.byref(frame), row0, nrows, out.ctypes.data if out.size else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_camera_rays: rows outside the image or an empty frame")
    return out


def camera_sample_rays(frame, sample, row0=0, nrows=None):
    """rtu_camera_sample_rays (pure host code): the primary rays and keys of sample `sample` of the recipe S frame `frame`, image rows
    [row0, row0 + nrows): (rays [nrows * width] of ray_dtype(), keys uint32 [nrows * width]) in image order — Halton pixel offset,
    lens point and sample_key(pixel, sample) as the renders draw them, bit for bit."""
    import numpy as np
    if nrows is None:
        nrows = frame.height - row0
    n = max(nrows, 0) * max(frame.width, 0)
    rays, keys = np.zeros(n, ray_dtype()), np.zeros(n, np.uint32)
    rc = hip.rtu_camera_sample_rays(ctypes.byref(frame), sample, row0, nrows, rays.ctypes.data if n else None, keys.ctypes.data if n else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_camera_sample_rays: not a recipe S frame, sample outside [0, samples) or rows outside the image")
    return rays, keys


def irradiance_desc(min_subdiv=None, max_subdiv=None, samples=None, first_sample=None, threshold_color=None, threshold_z=None, threshold_n=None,
                    max_bounce=None):
    """An RtuIrradianceDesc: rtu_irradiance_defaults (min_subdiv -5, max_subdiv 0, 64 samples, thresholds 1e30 / 1e30 / 0.7), then
    whatever is given. threshold_color: one number or three."""
    d = RtuIrradianceDesc()
    hip.rtu_irradiance_defaults(ctypes.byref(d))
    for name, v in (("min_subdiv", min_subdiv), ("max_subdiv", max_subdiv), ("samples", samples), ("first_sample", first_sample),
                    ("threshold_z", threshold_z), ("threshold_n", threshold_n), ("max_bounce", max_bounce)):
        if v is not None:
            setattr(d, name, v)
    if threshold_color is not None:
        tc = [float(threshold_color)] * 3 if not hasattr(threshold_color, "__len__") else [float(x) for x in threshold_color]
        d.threshold_color[:] = tc
    return d


def irradiance_grid(desc, width, height):
    """rtu_irradiance_grid (pure host code): (grid_w, grid_h, passes) of the map of a width x height image."""
    gw, gh, np_ = _I(), _I(), _I()
    rc = hip.rtu_irradiance_grid(ctypes.byref(desc), width, height, ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(np_))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_irradiance_grid: a descriptor outside its rules, or an image that is no multiple of 2^-max_subdiv")
    return gw.value, gh.value, np_.value


def irradiance_rays(frame, desc):
    """rtu_irradiance_rays (pure host code): the pinhole rays through all grid points of the map of `frame`, index order, as a
    structured array of ray_dtype()."""
    import numpy as np
    gw, gh, _ = irradiance_grid(desc, frame.width, frame.height)
    out = np.zeros(gw * gh, ray_dtype())
    rc = hip.rtu_irradiance_rays(ctypes.byref(frame), ctypes.byref(desc), out.ctypes.data)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_irradiance_rays")
    return out


def irradiance_classify(desc, width, height, pass_index, records, computed):
    """rtu_irradiance_classify (pure host code): one pass over records float32 [grid_h, grid_w, 8] and computed uint8 [grid_h, grid_w],
    both updated IN PLACE for the points the pass estimates. -> (visit uint32 [n]: the points in visiting order, compute bool [n]:
    which of them the pass wants computed; visit[compute] is its list)."""
    import numpy as np
    gw, gh, _ = irradiance_grid(desc, width, height)
    if records.dtype != np.float32 or not records.flags.c_contiguous or records.size != gw * gh * 8 or not records.flags.writeable:
        raise RtuError(RTU_ERR_ARG, "records: a writable contiguous float32 array of grid_h * grid_w * 8")
    if computed.dtype != np.uint8 or not computed.flags.c_contiguous or computed.size != gw * gh or not computed.flags.writeable:
        raise RtuError(RTU_ERR_ARG, "computed: a writable contiguous uint8 array of grid_h * grid_w")
    visit, comp, n = np.zeros(gw * gh, np.uint32), np.zeros(gw * gh, np.uint8), ctypes.c_uint32()
    rc = hip.rtu_irradiance_classify(ctypes.byref(desc), width, height, pass_index, records.ctypes.data, computed.ctypes.data, visit.ctypes.data,
                                     comp.ctypes.data, ctypes.byref(n))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_irradiance_classify: a descriptor outside its rules or a pass outside [0, passes)")
    return visit[:n.value].copy(), comp[:n.value].astype(bool)


def _irradiance_map(width, height, max_subdiv, records_ptr):
    m = RtuIrradianceMap()
    m.width, m.height, m.max_subdiv, m.records = width, height, max_subdiv, records_ptr
    return m


def irradiance_sample(records, width, height, max_subdiv, xy):
    """rtu_irradiance_sample (pure host code): the bilinear lookup of the map `records` (float32, grid_h * grid_w * 8) of a width x
    height image at image positions xy float32 [n, 2] -> float32 [n, 8] {E.rgb, z, N.xyz, 0}."""
    import numpy as np
    rec = np.ascontiguousarray(records, np.float32)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    out = np.zeros((len(xy), 8), np.float32)
    m = _irradiance_map(width, height, max_subdiv, rec.ctypes.data)
    rc = hip.rtu_irradiance_sample(ctypes.byref(m), xy.ctypes.data if len(xy) else None, len(xy), out.ctypes.data if len(xy) else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_irradiance_sample: an image that is no multiple of 2^-max_subdiv, or max_subdiv > 0")
    return out


def sample_key(pixel, sample):
    """rtu_sample_key: the key of the root Shade() call of sample `sample` of pixel `pixel` (include/rtu_render.h, sample streams)."""
    return int(hip.rtu_sample_key(int(pixel) & 0xFFFFFFFF, int(sample) & 0xFFFFFFFF))


def child_key(key, slot):
    """rtu_child_key: the key of the Shade() call behind secondary ray `slot` of the call with key `key`."""
    return int(hip.rtu_child_key(int(key) & 0xFFFFFFFF, int(slot) & 0xFFFFFFFF))


def scene_sort_box(scene):
    """rtu_scene_sort_box (pure host code): the box Context.ray_sort_box() reports once `scene` is uploaded, float32 [6]."""
    import numpy as np
    b = (ctypes.c_float * 6)()
    rc = hip.rtu_scene_sort_box(scene.desc_ptr, b)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_scene_sort_box: the scene does not validate")
    return np.array(list(b), np.float32)


def ray_sort_keys(box, rays):
    """rtu_ray_sort_keys (pure host code): the sort keys of `rays` (as for trace_rays) in `box` = (lo x, y, z, hi x, y, z) — what
    Context.ray_sort_box() returns for an uploaded scene — as uint32 [n]: 12 bits of Morton-coded cell of the point where the ray
    enters the box, 18 bits of Morton-coded octahedral direction; RTU_SORTKEY_MISS | the direction bits for a ray that misses the box, RTU_SORTKEY_INVALID
    for one the queries do not trace. The kernel's binary32 expressions in the same order: the same bits."""
    import numpy as np
    r = _as_rays(rays)
    b = (ctypes.c_float * 6)(*[float(x) for x in np.asarray(box, np.float32).reshape(6)])
    out = np.zeros(r.size, np.uint32)
    rc = hip.rtu_ray_sort_keys(b, r.ctypes.data if r.size else None, r.size, out.ctypes.data if r.size else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_ray_sort_keys")
    return out


def _as_keys(keys, n):
    import numpy as np
    k = np.ascontiguousarray(keys, np.uint32).reshape(-1)
    if k.size != n:
        raise RtuError(RTU_ERR_ARG, "keys: one uint32 per ray")
    return k


# the arrays of a mesh dump (include/rtu_render.h RTU_MESH_*): name -> (which, numpy dtype, trailing shape)
MESH_ARRAYS = {"bvh4": (0, "float32", (8, 4)), "bvh8": (1, "float32", (16, 4)), "fast_tri": (2, "float32", (4, 4)), "ref_tri": (3, "float32", (4, 4)),
               "ref_bvh": (4, "uint32", (8,)), "ref_elements": (5, "uint32", ()), "v": (6, "float32", (3,)), "vn": (7, "float32", (3,)),
               "header": (8, "uint32", ()), "fast_elements": (9, "uint32", ())}


def _mesh_dump(call, what):
    """Every array of MESH_ARRAYS through `call(which, out, capacity, bytes_out)` as a dict of numpy arrays. Nodes of bvh4 / bvh8 come as
    [nodes, 8 or 16, 4] float32 (view as uint32 for the ref words), ref_bvh as [nodes, 8] uint32 words {bmin, index, bmax, count}; the
    header is unpacked into bmin, bmax, scale (float32) and n_bvh_nodes, any_empty_box."""
    import numpy as np
    out = {}
    for name, (which, dtype, tail) in MESH_ARRAYS.items():
        n = ctypes.c_size_t(0)
        call(which, None, 0, ctypes.byref(n))  # the size (the call itself answers RTU_ERR_ARG: nothing fits in no buffer)
        buf = np.empty(n.value // 4, dtype)
        rc = call(which, buf.ctypes.data, buf.nbytes, ctypes.byref(n))
        if rc != RTU_OK:
            raise RtuError(rc, "%s: %s" % (what, name))
        out[name] = buf.reshape((-1,) + tail) if tail else buf
    h = out.pop("header")
    out["bmin"], out["bmax"], out["scale"] = h[0:3].view(np.float32), h[3:6].view(np.float32), h[6:7].view(np.float32)[0]
    out["n_bvh_nodes"], out["any_empty_box"] = int(h[7]), int(h[8])
    return out


def host_mesh(uploaded, mesh, now=None):
    """Pure host code (rtu_debug_host_mesh): what the device holds for mesh `mesh` after upload(uploaded) and update_meshes(now, [mesh]) —
    the fast tree's topology from `uploaded`, boxes / records / `ref` tree from `now`; now None: as upload(uploaded) builds it."""
    size = ctypes.sizeof(RtuMesh)
    up = uploaded.desc.meshes + mesh * size
    nw = now.desc.meshes + mesh * size if now is not None else None
    return _mesh_dump(lambda which, out, cap, n: hip.rtu_debug_host_mesh(up, nw, which, out, cap, n), "rtu_debug_host_mesh")


def host_ref_build(uploaded, mesh, v=None):
    """Pure host code (rtu_debug_host_ref_build): the host form of the device builder of rtu_update_meshes_device on the connectivity
    of mesh `mesh` of `uploaded` with the vertices v [nv, 3] (None: its own). A dict: ref_bvh [nodes, 8] uint32 words, ref_elements,
    vn (the recomputed normals; only where the mesh has one normal per vertex), bmin, bmax, scale, n_bvh_nodes, any_empty_box,
    bvh_depth. No depth bound."""
    import numpy as np
    m = uploaded.mesh(mesh)
    up = uploaded.desc.meshes + mesh * ctypes.sizeof(RtuMesh)
    vv = None
    if v is not None:
        vv = np.ascontiguousarray(v, np.float32)
        if vv.size != 3 * m.nv:
            raise RtuError(RTU_ERR_ARG, "host_ref_build: v is not [nv, 3]")
    out = {}
    arrays = {"ref_bvh": (4, "uint32", (8,)), "ref_elements": (5, "uint32", ()), "header": (8, "uint32", ())}
    if m.nvn == m.nv:
        arrays["vn"] = (7, "float32", (3,))
    for name, (which, dtype, tail) in arrays.items():
        n = ctypes.c_size_t(0)
        hip.rtu_debug_host_ref_build(up, vv.ctypes.data if vv is not None else None, which, None, 0, ctypes.byref(n))
        buf = np.empty(n.value // 4, dtype)
        rc = hip.rtu_debug_host_ref_build(up, vv.ctypes.data if vv is not None else None, which, buf.ctypes.data, buf.nbytes, ctypes.byref(n))
        if rc != RTU_OK:
            raise RtuError(rc, "rtu_debug_host_ref_build: %s" % name)
        out[name] = buf.reshape((-1,) + tail) if tail else buf
    h = out.pop("header")
    out["bmin"], out["bmax"], out["scale"] = h[0:3].view(np.float32), h[3:6].view(np.float32), h[6:7].view(np.float32)[0]
    out["n_bvh_nodes"], out["any_empty_box"], out["bvh_depth"] = int(h[7]), int(h[8]), int(h[9])
    return out


def partition_rule(keep):
    """Pure host code (rtu_debug_partition_rule): the closed form of the builder's partition for the keep flags `keep`; out[i] is the
    position whose element ends at position i."""
    import numpy as np
    k = np.ascontiguousarray(keep, np.uint8).reshape(-1)
    out = np.full(k.size, 0xFFFFFFFF, np.uint32)
    rc = hip.rtu_debug_partition_rule(k.ctypes.data if k.size else None, k.size, out.ctypes.data if k.size else None)
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_debug_partition_rule")
    return out


def scene_shape_diff(a, b):
    """Pure host code: None when scene b has the shape of scene a (rtu_update_scene would take b after a), else the first difference."""
    buf = ctypes.create_string_buffer(256)
    rc = hip.rtu_scene_shape_diff(a.desc_ptr, b.desc_ptr, buf, len(buf))
    if rc == RTU_OK:
        return None
    if rc != RTU_ERR_SCENE_SHAPE:
        raise RtuError(rc, buf.value.decode())
    return buf.value.decode()


def _dump_dict(d):
    import numpy as np
    if not d.usable:
        return None
    n = d.G * d.G + 1
    return {"G": d.G, "point": bool(d.point), "X": np.array(list(d.X)), "Y": np.array(list(d.Y)), "Z": np.array(list(d.Z)), "L": np.array(list(d.L)),
            "u0": d.u0, "v0": d.v0, "su": d.su, "sv": d.sv, "node": d.node, "light": d.light,
            "cell_off": np.ctypeslib.as_array(d.cell_off, (n,)).copy(), "entry_face": np.ctypeslib.as_array(d.entry_face, (max(d.n_entries, 1),))[:d.n_entries].copy(),
            "entry_zmin": np.ctypeslib.as_array(d.entry_zmin, (max(d.n_entries, 1),))[:d.n_entries].copy()}


def light_list(scene, light_slot, cover_slot):
    """Pure host code: the occluder list of (non-ambient light, mesh node) as numpy arrays, or None when no list is usable from there:
    dict(G, point, X, Y, Z, L, u0, v0, su, sv, node, light, cell_off [G*G+1], entry_face, entry_zmin)."""
    import numpy as np
    d = RtuLightListDump()
    rc = hip.rtu_debug_light_list(scene.desc_ptr, light_slot, cover_slot, ctypes.byref(d))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_debug_light_list")
    try:
        if not d.usable:
            return None
        n = d.G * d.G + 1
        return {"G": d.G, "point": bool(d.point), "X": np.array(list(d.X)), "Y": np.array(list(d.Y)), "Z": np.array(list(d.Z)), "L": np.array(list(d.L)),
                "u0": d.u0, "v0": d.v0, "su": d.su, "sv": d.sv, "node": d.node, "light": d.light,
                "cell_off": np.ctypeslib.as_array(d.cell_off, (n,)).copy(), "entry_face": np.ctypeslib.as_array(d.entry_face, (max(d.n_entries, 1),))[:d.n_entries].copy(),
                "entry_zmin": np.ctypeslib.as_array(d.entry_zmin, (max(d.n_entries, 1),))[:d.n_entries].copy()}
    finally:
        hip.rtu_debug_light_list_free(ctypes.byref(d))


def device_info(device_id=0):
    """What hipGetDeviceProperties says about a GPU (dict), e.g. for the HBM peak of the roofline."""
    o = RtuDeviceInfo()
    rc = hip.rtu_device_info(device_id, ctypes.byref(o))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_device_info")
    return {"compute_units": o.compute_units, "clock_khz": o.clock_khz, "memory_clock_khz": o.memory_clock_khz, "memory_bus_bits": o.memory_bus_bits,
            "l2_bytes": o.l2_bytes, "hbm_bytes": o.hbm_bytes, "name": o.name.decode(), "arch": o.arch.decode()}

# ---- rtu_host.h --------------------------------------------------------------
HOST_SYMBOLS = ["rtu_scene_load_xml", "rtu_scene_clone", "rtu_scene_load_blob", "rtu_scene_load_blob_file",
                "rtu_scene_to_blob", "rtu_scene_save_blob_file", "rtu_blob_free", "rtu_scene_desc",
                "rtu_scene_set_resolution", "rtu_scene_free", "rtu_host_last_error", "rtu_image_create",
                "rtu_image_free", "rtu_image_width", "rtu_image_height", "rtu_image_pixels", "rtu_image_zbuffer",
                "rtu_image_zimage", "rtu_image_num_rendered", "rtu_image_is_done", "rtu_image_from_rgbz",
                "rtu_image_compute_zimg", "rtu_image_save_png", "rtu_image_save_zpng", "rtu_write_png",
                "rtu_begin_render", "rtu_begin_render_sampled", "rtu_begin_render_paths", "rtu_stop_render", "rtu_render_wait", "rtu_render_gather_kind", "rtu_render_job_free",
                "rtu_image_sample_count", "rtu_image_fill_sample_count", "rtu_image_compute_sample_count_img", "rtu_image_sample_count_image",
                "rtu_image_save_sample_count_png", "rtu_begin_render_adaptive", "rtu_scene_node_scale", "rtu_scene_node_rotate",
                "rtu_scene_node_translate", "rtu_scene_set_light", "rtu_begin_render_progressive", "rtu_scene_set_mesh_vertices",
                "rtu_scene_recompute_normals"]
_sig(host, "rtu_scene_load_xml", _P, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p)
_sig(host, "rtu_scene_clone", _P, _P)
_sig(host, "rtu_scene_load_blob", _P, _P, ctypes.c_size_t)
_sig(host, "rtu_scene_load_blob_file", _P, ctypes.c_char_p)
_sig(host, "rtu_scene_to_blob", _P, _P, ctypes.POINTER(ctypes.c_size_t))
_sig(host, "rtu_scene_save_blob_file", _I, _P, ctypes.c_char_p)
_sig(host, "rtu_blob_free", None, _P)
_sig(host, "rtu_scene_desc", ctypes.POINTER(RtuSceneDesc), _P)
_sig(host, "rtu_scene_set_resolution", None, _P, _I, _I)
_sig(host, "rtu_scene_free", None, _P)
_F = ctypes.c_float
_sig(host, "rtu_scene_node_scale", _I, _P, ctypes.c_uint32, _F, _F, _F)
_sig(host, "rtu_scene_node_rotate", _I, _P, ctypes.c_uint32, _F, _F, _F, _F)
_sig(host, "rtu_scene_node_translate", _I, _P, ctypes.c_uint32, _F, _F, _F)
_sig(host, "rtu_scene_set_light", _I, _P, ctypes.c_uint32, _P)
_sig(host, "rtu_scene_set_mesh_vertices", _I, _P, ctypes.c_uint32, _P, _P)
_sig(host, "rtu_scene_recompute_normals", _I, _P, ctypes.c_uint32)
_sig(host, "rtu_host_last_error", ctypes.c_char_p)
_sig(host, "rtu_image_create", _P, _I, _I)
_sig(host, "rtu_image_free", None, _P)
_sig(host, "rtu_image_width", _I, _P)
_sig(host, "rtu_image_height", _I, _P)
_sig(host, "rtu_image_pixels", _P, _P)
_sig(host, "rtu_image_zbuffer", _P, _P)
_sig(host, "rtu_image_zimage", _P, _P)
_sig(host, "rtu_image_num_rendered", _I, _P)
_sig(host, "rtu_image_is_done", _I, _P)
_sig(host, "rtu_image_from_rgbz", None, _P, _P, _I, _I)
_sig(host, "rtu_image_compute_zimg", None, _P)
_sig(host, "rtu_image_save_png", _I, _P, ctypes.c_char_p)
_sig(host, "rtu_image_save_zpng", _I, _P, ctypes.c_char_p)
_sig(host, "rtu_write_png", _I, ctypes.c_char_p, _P, _I, _I, _I)
_sig(host, "rtu_begin_render", _P, _P, _P, ctypes.POINTER(_I), _I, ctypes.c_char_p, ctypes.c_char_p)
_sig(host, "rtu_begin_render_sampled", _P, _P, _P, ctypes.POINTER(_I), _I, _I, ctypes.c_char_p, ctypes.c_char_p)
_sig(host, "rtu_begin_render_paths", _P, _P, _P, ctypes.POINTER(_I), _I, _I, ctypes.c_char_p, ctypes.c_char_p)
_sig(host, "rtu_stop_render", None, _P)
_sig(host, "rtu_render_wait", _I, _P)
_sig(host, "rtu_render_gather_kind", _I, _P)
_sig(host, "rtu_render_job_free", None, _P)
_sig(host, "rtu_image_sample_count", _P, _P)
_sig(host, "rtu_image_fill_sample_count", None, _P, _P, _I, _I)
_sig(host, "rtu_image_compute_sample_count_img", _I, _P)
_sig(host, "rtu_image_sample_count_image", _P, _P)
_sig(host, "rtu_image_save_sample_count_png", _I, _P, ctypes.c_char_p)
_sig(host, "rtu_begin_render_adaptive", _P, _P, _P, ctypes.POINTER(_I), _I, _I, _I, ctypes.POINTER(RtuAdaptiveDesc), ctypes.c_char_p, ctypes.c_char_p,
     ctypes.c_char_p)
PASS_DONE = ctypes.CFUNCTYPE(None, _P, _I, _I)  # RtuPassDone(user, samples_done, pass)
_sig(host, "rtu_begin_render_progressive", _P, _P, _P, ctypes.POINTER(_I), _I, _I, _I, ctypes.POINTER(RtuAdaptiveDesc), ctypes.POINTER(_I), _I,
     PASS_DONE, _P, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p)


class ProgressiveJob:
    """rtu_begin_render_progressive: the frame refined pass by pass into `image` on a host thread. on_pass(samples_done, pass) is
    called after every pass (from that thread). wait() returns the job's code (RTU_ERR_CANCELLED after stop(): the image then holds
    the last complete pass)."""

    def __init__(self, scene, image, device_ids, samples, gather_bounces=0, adaptive=None, passes=None, on_pass=None, result_png=None,
                 zbuffer_png=None, samplecount_png=None):
        devs = (_I * len(device_ids))(*device_ids)
        sched = (_I * len(passes))(*passes) if passes is not None else None
        self._cb = PASS_DONE(lambda user, done, k: on_pass(done, k)) if on_pass else PASS_DONE()
        enc = lambda p: p.encode() if p else None
        self._h = host.rtu_begin_render_progressive(scene._h, image._h, devs, len(device_ids), samples, gather_bounces,
                                                    ctypes.byref(adaptive) if adaptive is not None else None, sched,
                                                    len(passes) if passes is not None else 0, self._cb, None, enc(result_png), enc(zbuffer_png),
                                                    enc(samplecount_png))
        if not self._h:
            raise RtuError(RTU_ERR_ARG, host.rtu_host_last_error().decode())
        self._keep = (scene, image)

    def stop(self):
        host.rtu_stop_render(self._h)

    def wait(self):
        return host.rtu_render_wait(self._h)

    def close(self):
        if self._h:
            host.rtu_render_job_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    """Owned flattened scene (RtuScene*)."""

    def __init__(self, handle):
        if not handle:
            raise RtuError(RTU_ERR_ARG, host.rtu_host_last_error().decode())
        self._h = handle

    @classmethod
    def from_xml(cls, path, remap_from=None, remap_to=None):
        enc = lambda s: s.encode() if s is not None else None
        return cls(host.rtu_scene_load_xml(path.encode(), enc(remap_from), enc(remap_to)))

    @classmethod
    def from_blob_bytes(cls, data):
        buf = ctypes.create_string_buffer(data, len(data))
        return cls(host.rtu_scene_load_blob(ctypes.cast(buf, _P), len(data)))

    @classmethod
    def from_blob_file(cls, path):
        if path.endswith(".gz"):
            import gzip
            with gzip.open(path, "rb") as f:
                return cls.from_blob_bytes(f.read())
        return cls(host.rtu_scene_load_blob_file(path.encode()))

    def to_blob_bytes(self):
        n = ctypes.c_size_t(0)
        p = host.rtu_scene_to_blob(self.desc_ptr, ctypes.byref(n))
        if not p:
            raise RtuError(RTU_ERR_ARG, "serialisation failed")
        try:
            return ctypes.string_at(p, n.value)
        finally:
            host.rtu_blob_free(p)

    @property
    def desc(self):
        return host.rtu_scene_desc(self._h).contents

    @property
    def desc_ptr(self):
        return ctypes.cast(host.rtu_scene_desc(self._h), _P)

    def set_resolution(self, w, h):
        host.rtu_scene_set_resolution(self._h, w, h)

    def _ok(self, rc, what):
        if rc != 0:
            raise RtuError(RTU_ERR_ARG, what)

    def node_scale(self, node, sx, sy=None, sz=None):
        """One more Transformation::Scale on node `node` (then Context.update)."""
        self._ok(host.rtu_scene_node_scale(self._h, node, sx, sx if sy is None else sy, sx if sz is None else sz), "node_scale: bad node")

    def node_rotate(self, node, axis, degrees):
        """One more Transformation::Rotate about `axis` (normalised as the loader does), in degrees."""
        self._ok(host.rtu_scene_node_rotate(self._h, node, axis[0], axis[1], axis[2], degrees), "node_rotate: bad node")

    def node_translate(self, node, offset):
        """One more Transformation::Translate."""
        self._ok(host.rtu_scene_node_translate(self._h, node, offset[0], offset[1], offset[2]), "node_translate: bad node")

    def set_light(self, index, light):
        """Replace light `index` with an RtuLight-layout ctypes structure (a direct light's direction is normalised)."""
        self._ok(host.rtu_scene_set_light(self._h, index, ctypes.byref(light)), "set_light: bad index")

    def mesh(self, mesh):
        """The RtuMesh header of mesh `mesh` (a view: read it again after an edit)."""
        if not 0 <= mesh < self.desc.n_meshes:
            raise RtuError(RTU_ERR_ARG, "no mesh %d" % mesh)
        return ctypes.cast(self.desc.meshes, ctypes.POINTER(RtuMesh))[mesh]

    def mesh_vertices(self, mesh):
        """A copy of the positions of mesh `mesh`: float32 [nv, 3]."""
        import numpy as np
        m = self.mesh(mesh)
        return np.ctypeslib.as_array(ctypes.cast(m.v, ctypes.POINTER(ctypes.c_float)), (m.nv, 3)).copy()

    def set_mesh_vertices(self, mesh, v, vn=None):
        """New positions v [nv, 3] (and normals vn [nvn, 3], or None: they stay) on the loaded connectivity; bounding box and the
        reference's BVH are rebuilt as the loader builds them (then Context.update_meshes)."""
        import numpy as np
        m = self.mesh(mesh)
        v = np.ascontiguousarray(v, np.float32)
        if v.size != m.nv * 3:
            raise RtuError(RTU_ERR_ARG, "set_mesh_vertices: %d floats for %d vertices" % (v.size, m.nv))
        if vn is not None:
            vn = np.ascontiguousarray(vn, np.float32)
            if vn.size != m.nvn * 3:
                raise RtuError(RTU_ERR_ARG, "set_mesh_vertices: %d floats for %d normals" % (vn.size, m.nvn))
        if host.rtu_scene_set_mesh_vertices(self._h, mesh, v.ctypes.data, vn.ctypes.data if vn is not None else None) != 0:
            raise RtuError(RTU_ERR_ARG, host.rtu_host_last_error().decode())

    def recompute_normals(self, mesh):
        """ComputeNormals from the current positions; only for a mesh whose normals have that form (one per vertex, fn == f)."""
        if host.rtu_scene_recompute_normals(self._h, mesh) != 0:
            raise RtuError(RTU_ERR_ARG, host.rtu_host_last_error().decode())

    def close(self):
        if self._h:
            host.rtu_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_setup(camera, width, height, shard_rank=0, shard_count=1, collect_stats=False, max_bounce=5, samples=0, gather_bounces=0):
    f = RtuFrameDesc()
    rc = hip.rtu_frame_setup(ctypes.byref(camera), width, height, ctypes.byref(f))
    if rc != RTU_OK:
        raise RtuError(rc, "rtu_frame_setup")
    f.shard_rank, f.shard_count = shard_rank, shard_count
    f.collect_stats = int(collect_stats)  # False / True, or 2: touched-bytes mode of the fast variant
    f.max_bounce = max_bounce
    f.samples = samples  # 0: recipe W; S >= 1: recipe S (soft shadows, glossy bounces, depth of field)
    f.gather_bounces = gather_bounces  # 4 (with samples): recipe P, + the Monte-Carlo gather of config 5
    return f


class MultiContext:
    """Several GPUs behind one handle (RtuMultiContext*): the frame sharded by interleaved 8-row bands, gathered and de-interleaved
    under the C-ABI. device_ids may repeat (several contexts on one GPU)."""

    def __init__(self, device_ids):
        err = _I(0)
        arr = (_I * len(device_ids))(*device_ids)
        self._h = hip.rtu_create_context_multi(arr, len(device_ids), ctypes.byref(err))
        if not self._h:
            raise RtuError(err.value, hip.rtu_error_string(err.value).decode())
        self.n = len(device_ids)

    def _check(self, rc):
        if rc != RTU_OK:
            raise RtuError(rc, hip.rtu_multi_last_error(self._h).decode())

    def upload(self, scene):
        self._check(hip.rtu_multi_upload_scene(self._h, scene.desc_ptr))

    def update(self, scene):
        """rtu_update_scene on every GPU's context: same shape, new placement / lights / materials / camera."""
        self._check(hip.rtu_multi_update_scene(self._h, scene.desc_ptr))

    def update_meshes(self, scene, meshes):
        """rtu_update_meshes on every GPU's context."""
        ids = (ctypes.c_uint32 * len(meshes))(*meshes)
        self._check(hip.rtu_multi_update_meshes(self._h, scene.desc_ptr, ids, len(meshes)))

    def context_handle(self, i):
        return hip.rtu_multi_context(self._h, i)

    def render(self, frame, on_rows=None, cancel=None):
        """The whole frame [H, W, 4] float32. on_rows(row0, nrows): called per band as the shards arrive; cancel: a ctypes.c_int the
        caller may set non-zero (the call then raises RtuError(RTU_ERR_CANCELLED))."""
        import numpy as np
        out = np.empty((frame.height, frame.width, 4), np.float32)
        prog = RtuProgress()
        cb = ROWS_DONE(lambda user, rows, row0, nrows: on_rows(row0, nrows)) if on_rows else ROWS_DONE()
        prog.rows_done = cb
        prog.cancel = ctypes.pointer(cancel) if cancel is not None else None
        self._check(hip.rtu_multi_render_frame(self._h, ctypes.byref(frame), out.ctypes.data, ctypes.byref(prog)))
        return out

    def gather_kind(self):
        return hip.rtu_multi_gather_kind(self._h)

    def close(self):
        if self._h:
            hip.rtu_destroy_context_multi(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Progressive:
    """A progressive session (RtuProgressive*, include/rtu_render.h): a recipe S / P frame refined call by call. Made by
    Context.progressive(); errors raise RtuError with the context's message."""

    def __init__(self, ctx, frame, adaptive=None):
        err = _I(0)
        self._ctx = ctx
        self.frame = frame
        self.adaptive = adaptive
        self._h = hip.rtu_progressive_begin(ctx._h, ctypes.byref(frame), ctypes.byref(adaptive) if adaptive is not None else None, ctypes.byref(err))
        if not self._h:
            ctx._check(err.value if err.value != RTU_OK else RTU_ERR_ARG)

    def _check(self, rc):
        if rc != RTU_OK:
            msg = hip.rtu_last_error(self._ctx._h).decode() if self._ctx._h else "the context is closed"
            raise RtuError(rc, msg)

    def advance(self, n, stream=None):
        """Trace the next n samples (synchronous)."""
        self._check(hip.rtu_progressive_advance(self._h, n, stream))

    def status(self):
        """(samples done, 8x8 tiles still sampling)."""
        done, live = ctypes.c_int32(0), ctypes.c_uint32(0)
        self._check(hip.rtu_progressive_status(self._h, ctypes.byref(done), ctypes.byref(live)))
        return done.value, live.value

    def snapshot(self):
        """The image now: (rgbz float32 [rows, W, 4], counts uint8 [rows, W] — the samples each pixel has — or None when frame.samples > 255)."""
        import numpy as np
        rows = hip.rtu_shard_rows(ctypes.byref(self.frame))
        out = np.empty((rows, self.frame.width, 4), np.float32)
        counts = np.empty((rows, self.frame.width), np.uint8) if self.frame.samples <= 255 else None
        self._check(hip.rtu_progressive_snapshot(self._h, out.ctypes.data, counts.ctypes.data if counts is not None else None))
        return out, counts

    def snapshot_device(self, d_rgbz, d_counts=None, stream=None):
        self._check(hip.rtu_progressive_snapshot_device(self._h, d_rgbz, d_counts, stream))

    def snapshot_denoised(self, desc=None):
        """The image now, filtered (rtu_progressive_snapshot_denoised): denoise(snapshot, frame_features of the session's frame) as
        float32 [H, W, 4]. desc: an RtuDenoiseDesc (None: the defaults). The features are made at the first call and kept."""
        import numpy as np
        out = np.empty((self.frame.height, self.frame.width, 4), np.float32)
        self._check(hip.rtu_progressive_snapshot_denoised(self._h, ctypes.byref(desc) if desc is not None else None, out.ctypes.data))
        return out

    def snapshot_denoised_device(self, d_rgbz, desc=None, stream=None):
        self._check(hip.rtu_progressive_snapshot_denoised_device(self._h, ctypes.byref(desc) if desc is not None else None, d_rgbz, stream))

    def close(self):
        if self._h:
            hip.rtu_progressive_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Temporal:
    """A temporal session (RtuTemporal*, include/rtu_render.h "Temporal accumulation"): one new sample per frame of a recipe S / P
    frame whose camera may move, accumulated by reprojection. Made by Context.temporal(); errors raise RtuError with the context's message.
    variance: an RtuVarianceDesc (see variance_desc()) makes it a variance session (rtu_temporal_begin_variance): its history holds the
    moments, and every frame is filtered by denoise_variance() with the variance() of that history. steer: an RtuSteerDesc (see
    steer_desc(); with variance) makes it a steered session (rtu_temporal_begin_steered): every frame spends steer.budget extra rays
    where that variance is highest and folds them into the history before it is filtered. gradient: an RtuGradientDesc (see
    gradient_desc(); with variance, steer or not) makes it a gradient session (rtu_temporal_begin_gradient): every frame re-shades one
    pixel per 3 x 3 stratum with the previous frame's random numbers and shortens the history where the shading changed. sparse: an
    RtuSparseDesc (see sparse_desc(); with variance, neither steer nor gradient) makes it a sparse session
    (rtu_temporal_begin_sparse): every frame shades one pixel of every block, the history carries the others. holes: an RtuHoleDesc
    (see hole_desc(); with sparse) makes that a sparse session with hole rays (rtu_temporal_begin_sparse_holes): every frame also
    shades up to holes.budget of the pixels that have no colour at all and makes the result their history."""

    def __init__(self, ctx, desc, variance=None, steer=None, gradient=None, sparse=None, holes=None):
        err = _I(0)
        self._ctx = ctx
        self.desc = desc
        if holes is not None and sparse is None:
            raise RtuError(RTU_ERR_ARG, "hole rays belong to a sparse session")
        if sparse is not None:
            if steer is not None or gradient is not None:
                raise RtuError(RTU_ERR_ARG, "a sparse session takes neither steer nor gradient")
            if holes is not None:
                self._h = hip.rtu_temporal_begin_sparse_holes(ctx._h, ctypes.byref(desc), ctypes.byref(variance) if variance is not None else None,
                                                              ctypes.byref(sparse), ctypes.byref(holes), ctypes.byref(err))
            else:
                self._h = hip.rtu_temporal_begin_sparse(ctx._h, ctypes.byref(desc), ctypes.byref(variance) if variance is not None else None,
                                                        ctypes.byref(sparse), ctypes.byref(err))
        elif gradient is not None:
            self._h = hip.rtu_temporal_begin_gradient(ctx._h, ctypes.byref(desc), ctypes.byref(variance) if variance is not None else None,
                                                      ctypes.byref(steer) if steer is not None else None, ctypes.byref(gradient), ctypes.byref(err))
        elif steer is not None:
            self._h = hip.rtu_temporal_begin_steered(ctx._h, ctypes.byref(desc), ctypes.byref(variance) if variance is not None else None,
                                                     ctypes.byref(steer), ctypes.byref(err))
        elif variance is not None:
            self._h = hip.rtu_temporal_begin_variance(ctx._h, ctypes.byref(desc), ctypes.byref(variance), ctypes.byref(err))
        else:
            self._h = hip.rtu_temporal_begin(ctx._h, ctypes.byref(desc), ctypes.byref(err))
        if not self._h:
            ctx._check(err.value if err.value != RTU_OK else RTU_ERR_ARG)

    def _check(self, rc):
        if rc != RTU_OK:
            msg = hip.rtu_last_error(self._ctx._h).decode() if self._ctx._h else "the context is closed"
            raise RtuError(rc, msg)

    def frame(self, frame):
        """The next frame of the session through the camera of `frame`: rgbz float32 [H, W, 4] (synchronous)."""
        import numpy as np
        out = np.empty((self.desc.height, self.desc.width, 4), np.float32)
        self._check(hip.rtu_temporal_frame(self._h, ctypes.byref(frame), out.ctypes.data))
        return out

    def frame_device(self, frame, d_rgbz, stream=None):
        self._check(hip.rtu_temporal_frame_device(self._h, ctypes.byref(frame), d_rgbz, stream))

    def frame_moved(self, frame, motion, history_cap=0):
        """The next frame after the scene was updated (Context.update / update_meshes): the history is kept and looked up through
        `motion`, scene_motion(scene of the previous frame, scene now). rgbz float32 [H, W, 4] (synchronous)."""
        import numpy as np
        motion = _as_motion(motion)
        out = np.empty((self.desc.height, self.desc.width, 4), np.float32)
        self._check(hip.rtu_temporal_frame_moved(self._h, ctypes.byref(frame), motion.ctypes.data, len(motion), int(history_cap), out.ctypes.data))
        return out

    def frame_moved_device(self, frame, motion, d_rgbz, history_cap=0, stream=None):
        motion = _as_motion(motion)
        self._check(hip.rtu_temporal_frame_moved_device(self._h, ctypes.byref(frame), motion.ctypes.data, len(motion), int(history_cap), d_rgbz, stream))

    def frame_deformed(self, frame, motion, history_cap=0):
        """frame_moved() that follows deforming meshes (rtu_temporal_frame_deformed): `motion` is scene_motion(previous scene, scene
        now, deform_meshes=[...]) — the meshes given to the ONE update_meshes since the previous frame —, the context has
        keep_previous_vertices(True); a plain, denoise or variance session. rgbz float32 [H, W, 4] (synchronous)."""
        import numpy as np
        motion = _as_motion(motion)
        out = np.empty((self.desc.height, self.desc.width, 4), np.float32)
        self._check(hip.rtu_temporal_frame_deformed(self._h, ctypes.byref(frame), motion.ctypes.data, len(motion), int(history_cap), out.ctypes.data))
        return out

    def frame_deformed_device(self, frame, motion, d_rgbz, history_cap=0, stream=None):
        motion = _as_motion(motion)
        self._check(hip.rtu_temporal_frame_deformed_device(self._h, ctypes.byref(frame), motion.ctypes.data, len(motion), int(history_cap), d_rgbz, stream))

    def sensor_frame(self, desc):
        """The next frame of the session through the sensor `desc` (an RtuSensorDesc of recipe S / P and of the session's size; a plain,
        denoise or variance session): rgbz float32 [H, W, 4] (synchronous). Camera and sensor frames may alternate: a frame after one
        of the other kind, or of another sensor model, takes no history."""
        import numpy as np
        out = np.empty((self.desc.height, self.desc.width, 4), np.float32)
        self._check(hip.rtu_temporal_sensor_frame(self._h, ctypes.byref(desc), out.ctypes.data))
        return out

    def sensor_frame_device(self, desc, d_rgbz, stream=None):
        self._check(hip.rtu_temporal_sensor_frame_device(self._h, ctypes.byref(desc), d_rgbz, stream))

    def history(self):
        """The history length of every pixel after the last frame, float32 [H, W] (0 before the first)."""
        import numpy as np
        n = self.desc.width * self.desc.height
        out = np.empty((self.desc.height, self.desc.width), np.float32)
        d = hip.rtu_device_alloc(self._ctx._h, 4 * n)
        if not d:
            self._check(RTU_ERR_HIP)
        try:
            self.history_device(d, hip.rtu_context_stream(self._ctx._h))
            self._check(hip.rtu_context_sync(self._ctx._h))
            self._check(hip.rtu_copy_to_host(self._ctx._h, out.ctypes.data, d, 4 * n))
        finally:
            hip.rtu_device_free(self._ctx._h, d)
        return out

    def history_device(self, d_n, stream=None):
        self._check(hip.rtu_temporal_history_device(self._h, d_n, stream))

    def lambda_image(self):
        """A gradient session: the lambda of every pixel's stratum in the last frame, float32 [H, W] (zeros where no gradient was taken)."""
        import numpy as np
        n = self.desc.width * self.desc.height
        out = np.empty((self.desc.height, self.desc.width), np.float32)
        d = hip.rtu_device_alloc(self._ctx._h, 4 * n)
        if not d:
            self._check(RTU_ERR_HIP)
        try:
            self.lambda_device(d, hip.rtu_context_stream(self._ctx._h))
            self._check(hip.rtu_context_sync(self._ctx._h))
            self._check(hip.rtu_copy_to_host(self._ctx._h, out.ctypes.data, d, 4 * n))
        finally:
            hip.rtu_device_free(self._ctx._h, d)
        return out

    def lambda_device(self, d_lambda, stream=None):
        self._check(hip.rtu_temporal_lambda_device(self._h, d_lambda, stream))

    def extra_counts(self):
        """A steered session: the extra rays every pixel got in the last frame, uint32 [H, W] (zeros before the first)."""
        import numpy as np
        n = self.desc.width * self.desc.height
        out = np.empty((self.desc.height, self.desc.width), np.uint32)
        d = hip.rtu_device_alloc(self._ctx._h, 4 * n)
        if not d:
            self._check(RTU_ERR_HIP)
        try:
            self.extra_counts_device(d, hip.rtu_context_stream(self._ctx._h))
            self._check(hip.rtu_context_sync(self._ctx._h))
            self._check(hip.rtu_copy_to_host(self._ctx._h, out.ctypes.data, d, 4 * n))
        finally:
            hip.rtu_device_free(self._ctx._h, d)
        return out

    def extra_counts_device(self, d_counts, stream=None):
        self._check(hip.rtu_temporal_extra_counts_device(self._h, d_counts, stream))

    def holes(self):
        """A sparse session: the number of pixels the last frame had no colour for and filled (0 before the first frame)."""
        n = _U32(0)
        self._check(hip.rtu_temporal_holes(self._h, ctypes.byref(n)))
        return int(n.value)

    def hole_rays(self):
        """A sparse session with hole rays: the number of hole rays of the last frame (0 before the first frame and with budget 0)."""
        n = _U32(0)
        self._check(hip.rtu_temporal_hole_rays(self._h, ctypes.byref(n)))
        return int(n.value)

    def steer_total(self):
        """A steered session: the number of extra rays of the last frame."""
        n = _U32(0)
        self._check(hip.rtu_temporal_steer_total(self._h, ctypes.byref(n)))
        return int(n.value)

    def reset(self):
        """Start over: the next frame is frame 0 and has no history."""
        self._check(hip.rtu_temporal_reset(self._h))

    def close(self):
        if self._h:
            hip.rtu_temporal_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One GPU (RtuContext*)."""

    def __init__(self, device_id=0):
        err = _I(0)
        self._h = hip.rtu_create_context(device_id, ctypes.byref(err))
        if not self._h:
            raise RtuError(err.value, hip.rtu_error_string(err.value).decode())

    def _check(self, rc):
        if rc != RTU_OK:
            raise RtuError(rc, hip.rtu_last_error(self._h).decode())

    def upload(self, scene):
        self._check(hip.rtu_upload_scene(self._h, scene.desc_ptr))

    def update(self, scene):
        """rtu_update_scene: the uploaded scene moved, relit or re-coloured (same shape); waits for launches in flight."""
        self._check(hip.rtu_update_scene(self._h, scene.desc_ptr))

    def update_meshes(self, scene, meshes):
        """rtu_update_meshes: update(scene), and the listed meshes take the vertices, normals and reference BVH of `scene` (same
        connectivity); the fast trees are refitted on the GPU."""
        ids = (ctypes.c_uint32 * len(meshes))(*meshes)
        self._check(hip.rtu_update_meshes(self._h, scene.desc_ptr, ids, len(meshes)))

    def update_meshes_device(self, scene, edits, stream=None):
        """rtu_update_meshes_device: update(scene), and the listed meshes take new vertices from DEVICE memory; the reference tree is
        rebuilt on the GPU. edits: {mesh: (d_v_ptr, d_vn_ptr or None, recompute_normals)} — raw device pointers (a torch tensor hands
        over .data_ptr()); stream: the stream the vertices were produced on (None: the default stream)."""
        arr = (RtuMeshDeviceEdit * max(len(edits), 1))()
        for i, (mesh, (d_v, d_vn, recompute)) in enumerate(edits.items()):
            arr[i].mesh, arr[i].flags, arr[i].d_v, arr[i].d_vn = mesh, RTU_MESH_EDIT_RECOMPUTE_NORMALS if recompute else 0, d_v, d_vn
        self._check(hip.rtu_update_meshes_device(self._h, scene.desc_ptr, arr, len(edits), stream))

    def mesh_shape(self, mesh):
        """rtu_context_mesh_shape: the header of mesh `mesh` as the context remembers it now (an RtuMesh with NULL arrays)."""
        h = RtuMesh()
        self._check(hip.rtu_context_mesh_shape(self._h, mesh, ctypes.byref(h)))
        return h

    def mesh_update_device_timing(self):
        """The ms update_meshes_device spent per phase since the previous call (enabled by mesh_update_timing())."""
        o = (ctypes.c_float * 4)()
        self._check(hip.rtu_debug_mesh_update_device_timing(self._h, o))
        return dict(zip(("build", "copies", "records_refit", "placement"), list(o)))

    def mesh_arrays(self, mesh):
        """What the context holds for mesh `mesh` now, copied back from the GPU: the dict of host_mesh()."""
        return _mesh_dump(lambda which, out, cap, n: hip.rtu_debug_context_mesh(self._h, mesh, which, out, cap, n), "rtu_debug_context_mesh")

    def mesh_update_timing(self, on=True):
        """Time the phases of later update_meshes calls; returns the ms spent per phase since the previous call."""
        o = (ctypes.c_float * 4)()
        self._check(hip.rtu_debug_mesh_update_timing(self._h, int(on), o))
        return dict(zip(("copies", "records", "refit", "placement"), list(o)))

    def light_list(self, index):
        """The occluder list the context holds now (index as in light_lists()), copied back: the dict of light_list()."""
        d = RtuLightListDump()
        self._check(hip.rtu_debug_context_light_list(self._h, index, ctypes.byref(d)))
        try:
            return _dump_dict(d)
        finally:
            hip.rtu_debug_light_list_free(ctypes.byref(d))

    def update_timing(self, on=True):
        """Time the device builder's phases in later updates; returns the ms spent per phase since the previous call."""
        o = (ctypes.c_float * 5)()
        self._check(hip.rtu_debug_update_timing(self._h, int(on), o))
        return dict(zip(("cover", "extent", "count", "fill", "sort"), list(o)))

    def render(self, frame, stats=False):
        """Render this shard; returns (rgbz float32 [rows, W, 4], stats dict or None)."""
        import numpy as np
        rows = hip.rtu_shard_rows(ctypes.byref(frame))
        out = np.empty((rows, frame.width, 4), np.float32)
        st = RtuStats() if stats else None
        self._check(hip.rtu_render_frame(self._h, ctypes.byref(frame), out.ctypes.data,
                                         ctypes.byref(st) if stats else None))
        return out, (st.as_dict() if stats else None)

    def render_device(self, frame, d_ptr, stream=None):
        self._check(hip.rtu_render_frame_device(self._h, ctypes.byref(frame), d_ptr, stream))

    def render_adaptive(self, frame, adaptive=None, stats=False):
        """Adaptive sampling (recipe S / P, frame.samples = the maximum per pixel): returns (rgbz float32 [rows, W, 4],
        counts uint8 [rows, W] — the samples each pixel took —, stats dict or None). adaptive: RtuAdaptiveDesc (None: the defaults)."""
        import numpy as np
        if adaptive is None:
            adaptive = adaptive_defaults()
        rows = hip.rtu_shard_rows(ctypes.byref(frame))
        out = np.empty((rows, frame.width, 4), np.float32)
        counts = np.empty((rows, frame.width), np.uint8)
        st = RtuStats() if stats else None
        self._check(hip.rtu_render_frame_adaptive(self._h, ctypes.byref(frame), ctypes.byref(adaptive), out.ctypes.data, counts.ctypes.data,
                                                  ctypes.byref(st) if stats else None))
        return out, counts, (st.as_dict() if stats else None)

    def progressive(self, frame, adaptive=None):
        """A progressive session of `frame` (recipe S / P; adaptive: RtuAdaptiveDesc or None for a fixed count): advance(n), status(),
        snapshot() -> (rgbz, counts), close()."""
        return Progressive(self, frame, adaptive)

    def temporal(self, desc, variance=None, steer=None, gradient=None, sparse=None, holes=None):
        """A temporal session (desc: an RtuTemporalDesc with the size of its frames, see temporal_desc()): frame(frame) -> rgbz,
        frame_device(), history(), reset(), close(). variance, steer, gradient, sparse, holes: see Temporal."""
        return Temporal(self, desc, variance, steer, gradient, sparse, holes)

    def hole_allocation_device(self, desc, d_hole_ptr, d_hits_ptr, d_counts_ptr, d_offsets_ptr, d_total_ptr, stream=None):
        """rtu_hole_allocation_device: hole_allocation() on device memory, the same words; the total is one uint32 at d_total_ptr."""
        self._check(hip.rtu_hole_allocation_device(self._h, ctypes.byref(desc), d_hole_ptr, d_hits_ptr, d_counts_ptr, d_offsets_ptr, d_total_ptr, stream))

    def hole_fold_device(self, desc, d_hist_ptr, d_rgbz_ptr, d_hole_ptr, d_hits_ptr, d_albedo_ptr, d_counts_ptr, d_offsets_ptr, d_rgbt_ptr, n_rays,
                         stream=None):
        """rtu_hole_fold_device: hole_fold() on device memory, in place in d_hist_ptr (four planes), d_rgbz_ptr and d_hole_ptr."""
        self._check(hip.rtu_hole_fold_device(self._h, ctypes.byref(desc), d_hist_ptr, d_rgbz_ptr, d_hole_ptr, d_hits_ptr, d_albedo_ptr, d_counts_ptr,
                                             d_offsets_ptr, d_rgbt_ptr, int(n_rays), stream))

    def sparse_rays_device(self, desc, frame, d_rays_ptr, d_keys_ptr, d_owner_ptr, stream=None):
        """rtu_sparse_rays_device: sparse_rays() written to device memory by a kernel, one ray, key and owner per block."""
        self._check(hip.rtu_sparse_rays_device(self._h, ctypes.byref(desc), ctypes.byref(frame), d_rays_ptr, d_keys_ptr, d_owner_ptr, stream))

    def temporal_accumulate_sparse_device(self, desc, sparse, prev_cam, cur_cam, d_rgbt_ptr, d_owner_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr,
                                          d_hist_out_ptr, d_rgbz_out_ptr, d_hole_ptr, d_motion_ptr, n_nodes, history_cap=0, stream=None):
        """rtu_temporal_accumulate_sparse_device: temporal_accumulate_sparse() on device memory; d_hole_ptr: width * height bytes."""
        self._check(hip.rtu_temporal_accumulate_sparse_device(self._h, ctypes.byref(desc), ctypes.byref(sparse),
                                                              ctypes.byref(prev_cam) if prev_cam is not None else None, ctypes.byref(cur_cam), d_rgbt_ptr,
                                                              d_owner_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr, d_rgbz_out_ptr,
                                                              d_hole_ptr, d_motion_ptr, n_nodes, int(history_cap), stream))

    def sparse_fill_device(self, desc, sparse, d_hits_ptr, d_albedo_ptr, d_owner_ptr, d_rgbt_ptr, d_hole_ptr, d_rgbz_ptr, stream=None):
        """rtu_sparse_fill_device: sparse_fill() on device memory, in place in d_rgbz_ptr."""
        self._check(hip.rtu_sparse_fill_device(self._h, ctypes.byref(desc), ctypes.byref(sparse), d_hits_ptr, d_albedo_ptr, d_owner_ptr, d_rgbt_ptr,
                                               d_hole_ptr, d_rgbz_ptr, stream))

    def gradient_rays_device(self, desc, frame, sample, d_rays_ptr, d_keys_ptr, d_owner_ptr, stream=None):
        """rtu_gradient_rays_device: gradient_rays() written to device memory by a kernel, one ray, key and owner per stratum."""
        self._check(hip.rtu_gradient_rays_device(self._h, ctypes.byref(desc), ctypes.byref(frame), int(sample), d_rays_ptr, d_keys_ptr, d_owner_ptr, stream))

    def sample_luminance_device(self, desc, d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_lum_ptr, stream=None):
        """rtu_sample_luminance_device: sample_luminance() on device memory, desc.width * desc.height floats to d_lum_ptr."""
        self._check(hip.rtu_sample_luminance_device(self._h, ctypes.byref(desc), d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_lum_ptr, stream))

    def temporal_gradient_device(self, desc, gradient, prev_cam, cur_cam, d_hits_ptr, d_albedo_ptr, d_motion_ptr, n_nodes, d_hist_prev_ptr, d_lum_prev_ptr,
                                 d_owner_ptr, d_rgbt_ptr, d_diff_ptr, d_lambda_ptr, stream=None):
        """rtu_temporal_gradient_device: temporal_gradient() on device memory: one float4 and one float per stratum."""
        self._check(hip.rtu_temporal_gradient_device(self._h, ctypes.byref(desc), ctypes.byref(gradient), ctypes.byref(prev_cam) if prev_cam is not None else None,
                                                     ctypes.byref(cur_cam), d_hits_ptr, d_albedo_ptr, d_motion_ptr, n_nodes, d_hist_prev_ptr, d_lum_prev_ptr,
                                                     d_owner_ptr, d_rgbt_ptr, d_diff_ptr, d_lambda_ptr, stream))

    def temporal_accumulate_gradient_device(self, desc, prev_cam, cur_cam, d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr,
                                            d_rgbz_out_ptr, d_motion_ptr, n_nodes, history_cap=0, d_lambda_ptr=None, stream=None):
        """rtu_temporal_accumulate_gradient_device: temporal_accumulate_gradient() on device memory; d_lambda_ptr: one float per stratum or None."""
        self._check(hip.rtu_temporal_accumulate_gradient_device(self._h, ctypes.byref(desc), ctypes.byref(prev_cam) if prev_cam is not None else None,
                                                                ctypes.byref(cur_cam), d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr,
                                                                d_rgbz_out_ptr, d_motion_ptr, n_nodes, int(history_cap), d_lambda_ptr, stream))

    def sample_allocation_device(self, desc, d_hist_ptr, d_hits_ptr, d_v_ptr, d_counts_ptr, d_offsets_ptr, d_total_ptr, stream=None):
        """rtu_sample_allocation_device: sample_allocation() on device memory, the same words; the total is one uint32 at d_total_ptr."""
        self._check(hip.rtu_sample_allocation_device(self._h, ctypes.byref(desc), d_hist_ptr, d_hits_ptr, d_v_ptr, d_counts_ptr, d_offsets_ptr,
                                                     d_total_ptr, stream))

    def extra_sample_rays_device(self, desc, frame, d_counts_ptr, d_offsets_ptr, capacity, d_rays_ptr, d_keys_ptr, d_owner_ptr, stream=None):
        """rtu_extra_sample_rays_device: extra_sample_rays() written to device memory by a kernel; nothing at or beyond `capacity`."""
        self._check(hip.rtu_extra_sample_rays_device(self._h, ctypes.byref(desc), ctypes.byref(frame), d_counts_ptr, d_offsets_ptr, int(capacity),
                                                     d_rays_ptr, d_keys_ptr, d_owner_ptr, stream))

    def temporal_refine_device(self, desc, d_hist_ptr, d_hits_ptr, d_albedo_ptr, d_counts_ptr, d_offsets_ptr, d_rgbt_ptr, n_rays, d_rgbz_ptr, stream=None):
        """rtu_temporal_refine_device: temporal_refine() on device memory, in place in d_hist_ptr (four planes) and d_rgbz_ptr."""
        self._check(hip.rtu_temporal_refine_device(self._h, ctypes.byref(desc), d_hist_ptr, d_hits_ptr, d_albedo_ptr, d_counts_ptr, d_offsets_ptr,
                                                   d_rgbt_ptr, int(n_rays), d_rgbz_ptr, stream))

    def camera_sample_rays_device(self, frame, sample, d_rays_ptr, d_keys_ptr, stream=None):
        """rtu_camera_sample_rays_device: the rays and keys of camera_sample_rays(frame, sample) written to device memory by a kernel."""
        self._check(hip.rtu_camera_sample_rays_device(self._h, ctypes.byref(frame), sample, d_rays_ptr, d_keys_ptr, stream))

    def temporal_accumulate_device(self, desc, prev_cam, cur_cam, d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr, d_rgbz_out_ptr,
                                   stream=None):
        """rtu_temporal_accumulate_device: temporal_accumulate() on device memory; d_hist_prev_ptr (and then prev_cam) may be None."""
        self._check(hip.rtu_temporal_accumulate_device(self._h, ctypes.byref(desc), ctypes.byref(prev_cam) if prev_cam is not None else None,
                                                       ctypes.byref(cur_cam), d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr,
                                                       d_rgbz_out_ptr, stream))

    def temporal_accumulate_motion_device(self, desc, prev_cam, cur_cam, d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr,
                                          d_rgbz_out_ptr, d_motion_ptr, n_nodes, history_cap=0, stream=None):
        """rtu_temporal_accumulate_motion_device: temporal_accumulate_motion() on device memory; d_motion_ptr: n_nodes RtuNodeMotion,
        16-byte aligned, trusted as it is."""
        self._check(hip.rtu_temporal_accumulate_motion_device(self._h, ctypes.byref(desc), ctypes.byref(prev_cam) if prev_cam is not None else None,
                                                              ctypes.byref(cur_cam), d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr,
                                                              d_rgbz_out_ptr, d_motion_ptr, n_nodes, int(history_cap), stream))

    def temporal_accumulate_moments_device(self, desc, prev_cam, cur_cam, d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr,
                                           d_rgbz_out_ptr, d_motion_ptr, n_nodes, history_cap=0, stream=None):
        """rtu_temporal_accumulate_moments_device: temporal_accumulate_moments() on device memory; the histories are four planes."""
        self._check(hip.rtu_temporal_accumulate_moments_device(self._h, ctypes.byref(desc), ctypes.byref(prev_cam) if prev_cam is not None else None,
                                                               ctypes.byref(cur_cam), d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr,
                                                               d_rgbz_out_ptr, d_motion_ptr, n_nodes, int(history_cap), stream))

    def temporal_accumulate_sensor_device(self, desc, prev, cur, d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr, d_rgbz_out_ptr,
                                          moments=False, stream=None):
        """rtu_temporal_accumulate_sensor_device / _sensor_moments_device: temporal_accumulate_sensor() on device memory, the same bits
        (k_temporal_sensor); the histories are three planes, with moments four. d_rgbz_out_ptr may be d_rgbz_ptr."""
        call = hip.rtu_temporal_accumulate_sensor_moments_device if moments else hip.rtu_temporal_accumulate_sensor_device
        self._check(call(self._h, ctypes.byref(desc), ctypes.byref(prev) if prev is not None else None, ctypes.byref(cur), d_rgbz_ptr, d_hits_ptr,
                         d_albedo_ptr, d_hist_prev_ptr, d_hist_out_ptr, d_rgbz_out_ptr, stream))

    def variance_device(self, desc, d_hist_ptr, d_hits_ptr, d_v_ptr, stream=None):
        """rtu_variance_device: variance() on device memory, desc.width * desc.height floats to d_v_ptr."""
        self._check(hip.rtu_variance_device(self._h, ctypes.byref(desc), d_hist_ptr, d_hits_ptr, d_v_ptr, stream))

    def denoise_variance_device(self, desc, d_in_ptr, d_hits_ptr, d_albedo_ptr, d_v_ptr, d_out_ptr, stream=None):
        """rtu_denoise_variance_device: denoise_variance() on device memory, the same bits; d_out_ptr may be d_in_ptr."""
        self._check(hip.rtu_denoise_variance_device(self._h, ctypes.byref(desc), d_in_ptr, d_hits_ptr, d_albedo_ptr, d_v_ptr, d_out_ptr, stream))

    def motion_vectors_device(self, desc, prev_cam, d_hits_ptr, d_motion_ptr, n_nodes, d_mv_ptr, stream=None):
        """rtu_motion_vectors_device: motion_vectors() on device memory, width * height float4 to d_mv_ptr."""
        self._check(hip.rtu_motion_vectors_device(self._h, ctypes.byref(desc), ctypes.byref(prev_cam), d_hits_ptr, d_motion_ptr, n_nodes, d_mv_ptr, stream))

    def keep_previous_vertices(self, on=True):
        """rtu_keep_previous_vertices: with it on, update_meshes keeps the positions and normals it replaces as the listed meshes'
        previous generation (what temporal_accumulate_deform_device reads); default off."""
        self._check(hip.rtu_keep_previous_vertices(self._h, 1 if on else 0))

    def temporal_accumulate_deform_device(self, desc, prev_cam, cur_cam, d_rgbz_ptr, d_hits_ptr, d_albedo_ptr, d_surface_ptr, d_hist_prev_ptr,
                                          d_hist_out_ptr, d_rgbz_out_ptr, d_motion_ptr, n_nodes, history_cap=0, moments=False, stream=None):
        """rtu_temporal_accumulate_deform_device / _deform_moments_device: temporal_accumulate_deform() on device memory, the same bits;
        connectivity and previous vertices are the context's own (keep_previous_vertices must be on); d_surface_ptr: the frame's
        RtuRaySurface records (frame_surface_device), 16-byte aligned."""
        call = hip.rtu_temporal_accumulate_deform_moments_device if moments else hip.rtu_temporal_accumulate_deform_device
        self._check(call(self._h, ctypes.byref(desc), ctypes.byref(prev_cam) if prev_cam is not None else None, ctypes.byref(cur_cam), d_rgbz_ptr,
                         d_hits_ptr, d_albedo_ptr, d_surface_ptr, d_hist_prev_ptr, d_hist_out_ptr, d_rgbz_out_ptr, d_motion_ptr, n_nodes,
                         int(history_cap), stream))

    def motion_vectors_deform_device(self, desc, prev_cam, d_hits_ptr, d_surface_ptr, d_motion_ptr, n_nodes, d_mv_ptr, stream=None):
        """rtu_motion_vectors_deform_device: motion_vectors_deform() on device memory, width * height float4 to d_mv_ptr."""
        self._check(hip.rtu_motion_vectors_deform_device(self._h, ctypes.byref(desc), ctypes.byref(prev_cam), d_hits_ptr, d_surface_ptr, d_motion_ptr,
                                                         n_nodes, d_mv_ptr, stream))

    def set_cancel(self, flag):
        """rtu_set_cancel_flag: a ctypes.c_int the library polls between sample batches (None: none)."""
        self._cancel = flag
        self._check(hip.rtu_set_cancel_flag(self._h, ctypes.byref(flag) if flag is not None else None))

    def sample_images(self, frame, first, n):
        """The images of samples [first, first + n) of the fixed recipe S / P frame: float32 [n, rows, W, 4], what the accumulator adds."""
        import numpy as np
        rows = hip.rtu_shard_rows(ctypes.byref(frame))
        out = np.empty((n, rows, frame.width, 4), np.float32)
        self._check(hip.rtu_debug_sample_images(self._h, ctypes.byref(frame), first, n, out.ctypes.data))
        return out

    def texcoords(self, op, x, index=0):
        """The kernels' texture arithmetic (TEXOP_*) on the inputs x (float32, TEXOP_IN[op] per input, any leading shape):
        float32 [n, TEXOP_OUT[op]] (n for ATAN2F / ASINF). TEXTURE / MAP read texture / map `index` of the uploaded scene."""
        import numpy as np
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        n = x.size // TEXOP_IN[op]
        out = np.empty((n, TEXOP_OUT[op]) if TEXOP_OUT[op] > 1 else (n,), np.float32)
        self._check(hip.rtu_debug_texcoords(self._h, op, index, x.ctypes.data, n, out.ctypes.data))
        return out

    def ray_sort_box(self):
        """rtu_ray_sort_box: the box the sort keys of this context's scene are quantised in, float32 [6] = lo x, y, z, hi x, y, z."""
        import numpy as np
        b = (ctypes.c_float * 6)()
        self._check(hip.rtu_ray_sort_box(self._h, b))
        return np.array(list(b), np.float32)

    def ray_order(self, rays):
        """rtu_ray_order: the permutation (uint32 [n]) that sorts `rays` by their sort key in this scene's box, stably — equal to
        np.argsort(ray_sort_keys(self.ray_sort_box(), rays), kind="stable"), computed on the GPU. rays[order] is the coherent batch."""
        import numpy as np
        r = _as_rays(rays)
        out = np.zeros(r.size, np.uint32)
        self._check(hip.rtu_ray_order(self._h, r.ctypes.data if r.size else None, r.size, out.ctypes.data if r.size else None))
        return out

    def ray_order_device(self, d_rays_ptr, n, d_order_ptr, stream=None):
        """rtu_ray_order_device: n RtuRay at d_rays_ptr -> the sorting permutation, n uint32 at d_order_ptr (device memory),
        asynchronous on `stream`. Uses scratch of the context: one stream per context."""
        self._check(hip.rtu_ray_order_device(self._h, d_rays_ptr, n, d_order_ptr, stream))

    def permute_device(self, d_src_ptr, d_dst_ptr, d_order_ptr, n, elem_bytes, scatter=False, stream=None):
        """rtu_permute_device: dst[i] = src[order[i]] (scatter False) or dst[order[i]] = src[i] (scatter True) for n elements of
        elem_bytes = 1, 4, 16, 32 or 48 in device memory, asynchronous on `stream`."""
        self._check(hip.rtu_permute_device(self._h, d_src_ptr, d_dst_ptr, d_order_ptr, n, elem_bytes, 1 if scatter else 0, stream))

    def _sorted(self, r, keys, out, call, shading):
        """sort=True of the five ray entries: upload the rays (and keys) once, order them on the GPU, gather them, run
        call(d_rays, d_keys, d_out, stream) — an existing _device entry, unchanged — on the sorted buffers, scatter the answers back to
        the callers' places and download them into `out`. A shading entry is repeated while rtu_frame_status reports
        RTU_ERR_CAPACITY, as its host form does, up to 8 times."""
        n = r.size
        if n == 0:
            return
        stream = hip.rtu_context_stream(self._h)
        ob = out.nbytes // n
        sizes = {"rays": 32 * n, "srays": 32 * n, "order": 4 * n, "sout": ob * n, "out": ob * n}
        if keys is not None:
            sizes.update(keys=4 * n, skeys=4 * n)
        d = {}
        try:
            for name, size in sizes.items():
                d[name] = hip.rtu_device_alloc(self._h, size)
                if not d[name]:
                    raise RtuError(RTU_ERR_HIP, "device allocation of %d bytes failed" % size)
            self._check(hip.rtu_copy_to_device(self._h, d["rays"], r.ctypes.data, 32 * n))
            if keys is not None:
                self._check(hip.rtu_copy_to_device(self._h, d["keys"], keys.ctypes.data, 4 * n))
            self._check(hip.rtu_ray_order_device(self._h, d["rays"], n, d["order"], stream))
            self._check(hip.rtu_permute_device(self._h, d["rays"], d["srays"], d["order"], n, 32, 0, stream))
            if keys is not None:
                self._check(hip.rtu_permute_device(self._h, d["keys"], d["skeys"], d["order"], n, 4, 0, stream))
            for attempt in range(8):
                call(d["srays"], d.get("skeys"), d["sout"], stream)
                if not shading:
                    break
                rc = hip.rtu_frame_status(self._h)
                if rc != RTU_ERR_CAPACITY:
                    self._check(rc)
                    break
            else:
                self._check(RTU_ERR_CAPACITY)
            self._check(hip.rtu_permute_device(self._h, d["sout"], d["out"], d["order"], n, ob, 1, stream))
            self._check(hip.rtu_context_sync(self._h))
            self._check(hip.rtu_copy_to_host(self._h, out.ctypes.data, d["out"], ob * n))
        finally:
            for ptr in d.values():
                if ptr:
                    hip.rtu_device_free(self._h, ptr)

    def trace_rays(self, rays, reference_walk=False, sort=False):
        """Closest hits of caller-supplied rays (rtu_trace_rays): rays float32 [n, 8] {org, tmax, dir, -} or a structured array of
        ray_dtype(); returns a structured array [n] of hit_dtype(). Directions must be of unit length (else RTU_RAY_INVALID).
        sort=True: the batch is brought into a coherent order on the GPU first (ray_order), traced by rtu_trace_rays_device, and the
        hits are put back in the callers' order: the same bytes. For the bare queries the sort costs more than it saves;
        it pays on the sampled and path-traced shading entries."""
        import numpy as np
        r = _as_rays(rays)
        out = np.zeros(r.size, hit_dtype())
        if sort:
            self._sorted(r, None, out, lambda dr, dk, do, st: self.trace_rays_device(dr, r.size, do, st, reference_walk=reference_walk), False)
            return out
        self._check(hip.rtu_trace_rays(self._h, r.ctypes.data if r.size else None, r.size, RTU_QUERY_REFERENCE_WALK if reference_walk else 0,
                                       out.ctypes.data if r.size else None))
        return out

    def occluded(self, rays, reference_walk=False, sort=False):
        """Is anything in front of tmax along each ray (rtu_occluded_rays)? uint8 [n], 1 or 0. sort=True: as for trace_rays."""
        import numpy as np
        r = _as_rays(rays)
        out = np.zeros(r.size, np.uint8)
        if sort:
            self._sorted(r, None, out, lambda dr, dk, do, st: self.occluded_device(dr, r.size, do, st, reference_walk=reference_walk), False)
            return out
        self._check(hip.rtu_occluded_rays(self._h, r.ctypes.data if r.size else None, r.size, RTU_QUERY_REFERENCE_WALK if reference_walk else 0,
                                          out.ctypes.data if r.size else None))
        return out

    occluded_rays = occluded  # the name of the C entry

    def trace_rays_device(self, d_rays_ptr, n, d_hits_ptr, stream=None, reference_walk=False, flags=None):
        """rtu_trace_rays_device: n RtuRay at d_rays_ptr -> n RtuRayHit at d_hits_ptr (device memory, 16-byte aligned: a torch tensor's
        data_ptr()), asynchronous on `stream`. flags (an integer) overrides reference_walk."""
        f = flags if flags is not None else (RTU_QUERY_REFERENCE_WALK if reference_walk else 0)
        self._check(hip.rtu_trace_rays_device(self._h, d_rays_ptr, n, f, d_hits_ptr, stream))

    def ray_features(self, rays, reference_walk=False):
        """First-hit features of caller-supplied rays (rtu_ray_features): rays as for trace_rays; returns (hits [n] of hit_dtype() — the
        bytes of trace_rays —, albedo float32 [n, 4] {r, g, b, 0}: the textured diffuse colour at a front-face hit, white for a node
        without a material, zero on a back face, at a miss and for an invalid ray)."""
        import numpy as np
        r = _as_rays(rays)
        hits, albedo = np.zeros(r.size, hit_dtype()), np.zeros((r.size, 4), np.float32)
        self._check(hip.rtu_ray_features(self._h, r.ctypes.data if r.size else None, r.size, RTU_QUERY_REFERENCE_WALK if reference_walk else 0,
                                         hits.ctypes.data if r.size else None, albedo.ctypes.data if r.size else None))
        return hits, albedo

    def ray_features_device(self, d_rays_ptr, n, d_hits_ptr, d_albedo_ptr, stream=None, reference_walk=False, flags=None):
        """rtu_ray_features_device: n RtuRay -> n RtuRayHit and n float4 albedo in device memory (16-byte aligned), asynchronous on `stream`."""
        f = flags if flags is not None else (RTU_QUERY_REFERENCE_WALK if reference_walk else 0)
        self._check(hip.rtu_ray_features_device(self._h, d_rays_ptr, n, f, d_hits_ptr, d_albedo_ptr, stream))

    def frame_features(self, frame):
        """rtu_frame_features: ray_features of the pixel-centre rays of `frame` (camera_rays(frame)), generated on the GPU:
        (hits [H * W], albedo float32 [H * W, 4]) in image order. frame.shard_count must be 1."""
        import numpy as np
        n = max(frame.width, 0) * max(frame.height, 0)
        hits, albedo = np.zeros(n, hit_dtype()), np.zeros((n, 4), np.float32)
        self._check(hip.rtu_frame_features(self._h, ctypes.byref(frame), hits.ctypes.data if n else None, albedo.ctypes.data if n else None))
        return hits, albedo

    def frame_features_device(self, frame, d_hits_ptr, d_albedo_ptr, stream=None):
        """rtu_frame_features_device: width * height RtuRayHit and float4 albedo into device memory, asynchronous on `stream`."""
        self._check(hip.rtu_frame_features_device(self._h, ctypes.byref(frame), d_hits_ptr, d_albedo_ptr, stream))

    def ray_surface(self, rays, reference_walk=False):
        """ray_features with the surface record of every ray (rtu_ray_surface): (hits, albedo, surface [n] of surface_dtype()). On a
        triangle-mesh hit surface holds the mesh, the face (an index into the mesh's f / fn / ft) and the weights of its three
        vertices that the hit point, normal and texture coordinate were interpolated with; mesh = face = -1 elsewhere. uvw is the
        hit's texture coordinate on every kind of object."""
        import numpy as np
        r = _as_rays(rays)
        hits, albedo, surface = np.zeros(r.size, hit_dtype()), np.zeros((r.size, 4), np.float32), np.zeros(r.size, surface_dtype())
        self._check(hip.rtu_ray_surface(self._h, r.ctypes.data if r.size else None, r.size, RTU_QUERY_REFERENCE_WALK if reference_walk else 0,
                                        hits.ctypes.data if r.size else None, albedo.ctypes.data if r.size else None,
                                        surface.ctypes.data if r.size else None))
        return hits, albedo, surface

    def ray_surface_device(self, d_rays_ptr, n, d_hits_ptr, d_albedo_ptr, d_surface_ptr, stream=None, reference_walk=False, flags=None):
        """rtu_ray_surface_device: ray_features_device and n RtuRaySurface at d_surface_ptr (16-byte aligned), asynchronous on `stream`."""
        f = flags if flags is not None else (RTU_QUERY_REFERENCE_WALK if reference_walk else 0)
        self._check(hip.rtu_ray_surface_device(self._h, d_rays_ptr, n, f, d_hits_ptr, d_albedo_ptr, d_surface_ptr, stream))

    def frame_surface(self, frame):
        """rtu_frame_surface: ray_surface of the pixel-centre rays of `frame`: (hits [H * W], albedo [H * W, 4], surface [H * W])."""
        import numpy as np
        n = max(frame.width, 0) * max(frame.height, 0)
        hits, albedo, surface = np.zeros(n, hit_dtype()), np.zeros((n, 4), np.float32), np.zeros(n, surface_dtype())
        self._check(hip.rtu_frame_surface(self._h, ctypes.byref(frame), hits.ctypes.data if n else None, albedo.ctypes.data if n else None,
                                          surface.ctypes.data if n else None))
        return hits, albedo, surface

    def frame_surface_device(self, frame, d_hits_ptr, d_albedo_ptr, d_surface_ptr, stream=None):
        """rtu_frame_surface_device: frame_features_device and width * height RtuRaySurface into device memory, asynchronous on `stream`."""
        self._check(hip.rtu_frame_surface_device(self._h, ctypes.byref(frame), d_hits_ptr, d_albedo_ptr, d_surface_ptr, stream))

    def denoise_device(self, desc, d_in_ptr, d_hits_ptr, d_albedo_ptr, d_out_ptr, stream=None):
        """rtu_denoise_device: the filter of denoise() on device memory (desc.width * desc.height float4 / RtuRayHit / float4), the same
        bits, asynchronous on `stream`; d_out_ptr may be d_in_ptr. Its planes are grow-only buffers of the context."""
        self._check(hip.rtu_denoise_device(self._h, ctypes.byref(desc), d_in_ptr, d_hits_ptr, d_albedo_ptr, d_out_ptr, stream))

    def shade_rays(self, rays, eye, max_bounce=5, reference_walk=False, stats=False, desc=None, sort=False):
        """Radiance along caller-supplied rays (rtu_shade_rays): rays as for trace_rays; eye is the camera position of Shade()'s view
        vector. Returns (float32 [n, 4] {r, g, b, t}, stats dict or None): a hit is shaded like a render's pixel, a miss is the
        environment along the ray with t = tmax, an invalid ray is four zeros. desc (an RtuShadeDesc) overrides the other options.
        sort=True: ordered on the GPU first (ray_order), shaded by the _device entry on the sorted batch, answers put back: the same bytes."""
        import numpy as np
        r = _as_rays(rays)
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        out = np.zeros((r.size, 4), np.float32)
        st = RtuStats() if stats else None
        if sort:
            if stats:
                raise RtuError(RTU_ERR_ARG, "sort=True goes through the _device entry, which returns no counters: stats=False")
            self._sorted(r, None, out, lambda dr, dk, do, st_: self.shade_rays_device(dr, r.size, eye, do, st_, desc=d), True)
            return out, None
        self._check(hip.rtu_shade_rays(self._h, r.ctypes.data if r.size else None, r.size, ctypes.byref(d), out.ctypes.data if r.size else None,
                                       ctypes.byref(st) if stats else None))
        return out, (st.as_dict() if stats else None)

    def shade_rays_device(self, d_rays_ptr, n, eye, d_rgbt_ptr, stream=None, max_bounce=5, reference_walk=False, desc=None):
        """rtu_shade_rays_device: n RtuRay at d_rays_ptr -> n float4 {r, g, b, t} at d_rgbt_ptr (device memory, 16-byte aligned),
        asynchronous on `stream`; frame_status() afterwards as for render_device (RTU_ERR_CAPACITY: call it again)."""
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        self._check(hip.rtu_shade_rays_device(self._h, d_rays_ptr, n, ctypes.byref(d), d_rgbt_ptr, stream))

    def shade_rays_sampled(self, rays, keys, eye, max_bounce=5, reference_walk=False, stats=False, desc=None, sort=False):
        """Recipe S along caller-supplied rays (rtu_shade_rays_sampled): as shade_rays, with one uint32 key per ray — the key of the
        sample streams of that ray's root Shade() call (soft shadows, glossy bounces). One sample per ray; scenes with stochastic
        features are accepted. Returns (float32 [n, 4] {r, g, b, t}, stats dict or None).
        sort=True: ordered on the GPU first (ray_order), shaded by the _device entry on the sorted batch, answers put back: the same bytes."""
        import numpy as np
        r = _as_rays(rays)
        k = _as_keys(keys, r.size)
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        out = np.zeros((r.size, 4), np.float32)
        st = RtuStats() if stats else None
        if sort:
            if stats:
                raise RtuError(RTU_ERR_ARG, "sort=True goes through the _device entry, which returns no counters: stats=False")
            self._sorted(r, k, out, lambda dr, dk, do, st_: self.shade_rays_sampled_device(dr, dk, r.size, eye, do, st_, desc=d), True)
            return out, None
        self._check(hip.rtu_shade_rays_sampled(self._h, r.ctypes.data if r.size else None, k.ctypes.data if r.size else None, r.size, ctypes.byref(d),
                                               out.ctypes.data if r.size else None, ctypes.byref(st) if stats else None))
        return out, (st.as_dict() if stats else None)

    def shade_rays_sampled_device(self, d_rays_ptr, d_keys_ptr, n, eye, d_rgbt_ptr, stream=None, max_bounce=5, reference_walk=False, desc=None):
        """rtu_shade_rays_sampled_device: n RtuRay at d_rays_ptr and n uint32 keys at d_keys_ptr -> n float4 {r, g, b, t} at d_rgbt_ptr
        (device memory), asynchronous on `stream`; frame_status() afterwards as for render_device."""
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        self._check(hip.rtu_shade_rays_sampled_device(self._h, d_rays_ptr, d_keys_ptr, n, ctypes.byref(d), d_rgbt_ptr, stream))

    def shade_rays_paths(self, rays, keys, eye, max_bounce=5, reference_walk=False, stats=False, desc=None, sort=False):
        """Recipe P along caller-supplied rays (rtu_shade_rays_paths): as shade_rays_sampled, with the 4-bounce Monte-Carlo gather
        behind every hit — rgb = Shade(hit, lights + the gathered AmbientLight) + Shade(hit, lights). keys[i] is the key of ray i's
        root call; the gather draws from it as a recipe-P frame does. Returns (float32 [n, 4] {r, g, b, t}, stats dict or None).
        sort=True: ordered on the GPU first (ray_order), shaded by the _device entry on the sorted batch, answers put back: the same bytes."""
        import numpy as np
        r = _as_rays(rays)
        k = _as_keys(keys, r.size)
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        out = np.zeros((r.size, 4), np.float32)
        st = RtuStats() if stats else None
        if sort:
            if stats:
                raise RtuError(RTU_ERR_ARG, "sort=True goes through the _device entry, which returns no counters: stats=False")
            self._sorted(r, k, out, lambda dr, dk, do, st_: self.shade_rays_paths_device(dr, dk, r.size, eye, do, st_, desc=d), True)
            return out, None
        self._check(hip.rtu_shade_rays_paths(self._h, r.ctypes.data if r.size else None, k.ctypes.data if r.size else None, r.size, ctypes.byref(d),
                                             out.ctypes.data if r.size else None, ctypes.byref(st) if stats else None))
        return out, (st.as_dict() if stats else None)

    def shade_rays_paths_device(self, d_rays_ptr, d_keys_ptr, n, eye, d_rgbt_ptr, stream=None, max_bounce=5, reference_walk=False, desc=None):
        """rtu_shade_rays_paths_device: n RtuRay at d_rays_ptr and n uint32 keys at d_keys_ptr -> n float4 {r, g, b, t} at d_rgbt_ptr
        (device memory, n <= 2^25), the whole sequence asynchronous on `stream`; frame_status() afterwards as for render_device
        (RTU_ERR_CAPACITY: call this again)."""
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        self._check(hip.rtu_shade_rays_paths_device(self._h, d_rays_ptr, d_keys_ptr, n, ctypes.byref(d), d_rgbt_ptr, stream))

    def gather_rays(self, rays, keys, eye, max_bounce=5, reference_walk=False, stats=False, desc=None):
        """rtu_gather_rays: the indirect half of a recipe-P sample — per ray {c.r, c.g, c.b, t}, c the intensity of the AmbientLight the
        4-bounce gather behind the ray's hit appends for its key (0 on a miss, an invalid ray, a node without material).
        Returns (float32 [n, 4], stats dict or None)."""
        import numpy as np
        r = _as_rays(rays)
        k = _as_keys(keys, r.size)
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        out = np.zeros((r.size, 4), np.float32)
        st = RtuStats() if stats else None
        self._check(hip.rtu_gather_rays(self._h, r.ctypes.data if r.size else None, k.ctypes.data if r.size else None, r.size, ctypes.byref(d),
                                        out.ctypes.data if r.size else None, ctypes.byref(st) if stats else None))
        return out, (st.as_dict() if stats else None)

    def gather_rays_device(self, d_rays_ptr, d_keys_ptr, n, eye, d_ct_ptr, stream=None, max_bounce=5, reference_walk=False, desc=None):
        """rtu_gather_rays_device: device memory, asynchronous on `stream`; frame_status() afterwards (RTU_ERR_CAPACITY: call this again)."""
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        self._check(hip.rtu_gather_rays_device(self._h, d_rays_ptr, d_keys_ptr, n, ctypes.byref(d), d_ct_ptr, stream))

    def shade_rays_ambient(self, rays, keys, amb, eye, max_bounce=5, reference_walk=False, stats=False, desc=None):
        """rtu_shade_rays_ambient: the direct half — a recipe-S ray batch whose root calls are lit by lights + AmbientLight(amb[i]);
        amb float32 [n, 4] {r, g, b, ignored} (what gather_rays returns) or [n, 3]. Returns (float32 [n, 4] {r, g, b, t}, stats or None)."""
        import numpy as np
        r = _as_rays(rays)
        k = _as_keys(keys, r.size)
        a = np.asarray(amb, np.float32).reshape(r.size, -1)
        if a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((r.size, 1), np.float32)], axis=1)
        if a.shape[1] != 4:
            raise RtuError(RTU_ERR_ARG, "amb: float32 [n, 4] or [n, 3]")
        a = np.ascontiguousarray(a)
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        out = np.zeros((r.size, 4), np.float32)
        st = RtuStats() if stats else None
        self._check(hip.rtu_shade_rays_ambient(self._h, r.ctypes.data if r.size else None, k.ctypes.data if r.size else None,
                                               a.ctypes.data if r.size else None, r.size, ctypes.byref(d), out.ctypes.data if r.size else None,
                                               ctypes.byref(st) if stats else None))
        return out, (st.as_dict() if stats else None)

    def shade_rays_ambient_device(self, d_rays_ptr, d_keys_ptr, d_amb_ptr, n, eye, d_rgbt_ptr, stream=None, max_bounce=5, reference_walk=False, desc=None):
        """rtu_shade_rays_ambient_device: device memory (amb n float4), asynchronous on `stream`; frame_status() afterwards."""
        d = desc if desc is not None else shade_desc(eye, max_bounce, reference_walk)
        self._check(hip.rtu_shade_rays_ambient_device(self._h, d_rays_ptr, d_keys_ptr, d_amb_ptr, n, ctypes.byref(d), d_rgbt_ptr, stream))

    def irradiance_build(self, frame, desc):
        """rtu_irradiance_build: the irradiance map of `frame` (its pinhole camera, width, height) -> (records float32 [grid_h, grid_w, 8]
        {E.rgb, z, N.xyz, 0}, computed uint8 [grid_h, grid_w], per_pass uint32 [passes, 2] {visited, computed})."""
        import numpy as np
        gw, gh, passes = irradiance_grid(desc, frame.width, frame.height)
        rec, comp, per = np.zeros((gh, gw, 8), np.float32), np.zeros((gh, gw), np.uint8), np.zeros((passes, 2), np.uint32)
        n = ctypes.c_uint32()
        self._check(hip.rtu_irradiance_build(self._h, ctypes.byref(frame), ctypes.byref(desc), rec.ctypes.data, comp.ctypes.data, ctypes.byref(n), per.ctypes.data))
        assert n.value == int(per[:, 1].sum())
        return rec, comp, per

    def irradiance_build_device(self, frame, desc, d_records_ptr, d_computed_ptr, stream=None):
        """rtu_irradiance_build_device: records (grid points x 32 B, 16-byte aligned) and bytes into device memory; returns when the map
        is complete on `stream`. -> per_pass uint32 [passes, 2]."""
        import numpy as np
        _, _, passes = irradiance_grid(desc, frame.width, frame.height)
        per = np.zeros((passes, 2), np.uint32)
        n = ctypes.c_uint32()
        self._check(hip.rtu_irradiance_build_device(self._h, ctypes.byref(frame), ctypes.byref(desc), d_records_ptr, d_computed_ptr, ctypes.byref(n),
                                                    per.ctypes.data, stream))
        return per

    def irradiance_sample_device(self, d_records_ptr, width, height, max_subdiv, d_xy_ptr, n, d_out_ptr, stream=None):
        """rtu_irradiance_sample_device: the lookup at n positions {px, py} in device memory -> n x 8 floats, asynchronous on `stream`."""
        m = _irradiance_map(width, height, max_subdiv, d_records_ptr)
        self._check(hip.rtu_irradiance_sample_device(self._h, ctypes.byref(m), d_xy_ptr, n, d_out_ptr, stream))

    def render_irradiance(self, frame, records, max_subdiv):
        """rtu_render_frame_irradiance: a recipe-S frame of frame.samples samples whose root calls also get the AmbientLight of the map
        `records` (as irradiance_build returns them) at the pixel's centre -> float32 [height, width, 4] {r, g, b, z}."""
        import numpy as np
        rec = np.ascontiguousarray(records, np.float32)
        out = np.zeros((frame.height, frame.width, 4), np.float32)
        m = _irradiance_map(frame.width, frame.height, max_subdiv, rec.ctypes.data)
        self._check(hip.rtu_render_frame_irradiance(self._h, ctypes.byref(frame), ctypes.byref(m), out.ctypes.data))
        return out

    def render_irradiance_device(self, frame, d_records_ptr, max_subdiv, d_rgbz_ptr, stream=None):
        """rtu_render_frame_irradiance_device: map records and image in device memory; returns when the image is complete on `stream`."""
        m = _irradiance_map(frame.width, frame.height, max_subdiv, d_records_ptr)
        self._check(hip.rtu_render_frame_irradiance_device(self._h, ctypes.byref(frame), ctypes.byref(m), d_rgbz_ptr, stream))

    def sensor_rays_device(self, desc, d_rays_ptr, d_keys_ptr=None, sample0=0, nsamples=1, stream=None):
        """rtu_sensor_rays_device: the rays (and keys, unless d_keys_ptr is None) of samples [sample0, sample0 + nsamples) of the
        sensor into device memory, sample-major — ray (k - sample0) * width * height + pixel —, the bits of sensor_rays, asynchronous
        on `stream`. Needs no scene."""
        self._check(hip.rtu_sensor_rays_device(self._h, ctypes.byref(desc), sample0, nsamples, d_rays_ptr, d_keys_ptr, stream))

    def render_sensor(self, desc):
        """rtu_render_sensor: the image of the sensor, float32 [height, width, 4] {r, g, b, z} (what Image.fill accepts): per pixel
        the mean of its samples in sample order, z the mean t of the samples that hit (RTU_BIGFLOAT when none did)."""
        import numpy as np
        out = np.empty((max(desc.height, 0), max(desc.width, 0), 4), np.float32)
        self._check(hip.rtu_render_sensor(self._h, ctypes.byref(desc), out.ctypes.data if out.size else None))
        return out

    def render_sensor_device(self, desc, d_ptr, stream=None):
        """rtu_render_sensor_device: the same image into device memory (height * width float4 at d_ptr, 16-byte aligned), the
        launches on `stream`; returns when the image is complete."""
        self._check(hip.rtu_render_sensor_device(self._h, ctypes.byref(desc), d_ptr, stream))

    def render_sensor_adaptive(self, desc, adaptive=None):
        """rtu_render_sensor_adaptive: the sensor (recipe S / P, desc.samples = the maximum per pixel, 1 .. 255) sampled until each
        pixel's samples agree: (rgbz float32 [height, width, 4], counts uint8 [height, width] — the samples each pixel took).
        adaptive: RtuAdaptiveDesc (None: the defaults)."""
        import numpy as np
        if adaptive is None:
            adaptive = adaptive_defaults()
        out = np.empty((max(desc.height, 0), max(desc.width, 0), 4), np.float32)
        counts = np.empty(out.shape[:2], np.uint8)
        self._check(hip.rtu_render_sensor_adaptive(self._h, ctypes.byref(desc), ctypes.byref(adaptive), out.ctypes.data if out.size else None,
                                                   counts.ctypes.data if counts.size else None))
        return out, counts

    def render_sensor_adaptive_device(self, desc, d_rgbz, d_counts=None, adaptive=None, stream=None):
        """rtu_render_sensor_adaptive_device: the same into device memory (height * width float4 at d_rgbz, 16-byte aligned; height *
        width bytes at d_counts unless None), the launches on `stream`; returns when the image is complete."""
        if adaptive is None:
            adaptive = adaptive_defaults()
        self._check(hip.rtu_render_sensor_adaptive_device(self._h, ctypes.byref(desc), ctypes.byref(adaptive), d_rgbz, d_counts, stream))

    def sensor_adaptive_trace(self):
        """rtu_debug_sensor_adaptive_trace: [(live pixels, samples)] of every batch of the last adaptive sensor render of this context."""
        n = hip.rtu_debug_sensor_adaptive_trace(self._h, None, None, 0)
        self._check(min(n, 0))
        live, batch = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint32 * max(n, 1))()
        self._check(min(hip.rtu_debug_sensor_adaptive_trace(self._h, live, batch, n), 0))
        return [(int(live[b]), int(batch[b])) for b in range(n)]

    def sensor_timing(self, on=True):
        """Time the kernels of later sensor renders; returns the ms spent since the previous call in k_sensor_rays, in
        k_sensor_accumulate and in the renders as a whole."""
        o = (ctypes.c_float * 3)()
        self._check(hip.rtu_debug_sensor_timing(self._h, int(on), o))
        return dict(zip(("rays", "accumulate", "render"), list(o)))

    def occluded_device(self, d_rays_ptr, n, d_occluded_ptr, stream=None, reference_walk=False, flags=None):
        """rtu_occluded_rays_device: n RtuRay at d_rays_ptr -> n bytes (1 / 0) at d_occluded_ptr, asynchronous on `stream`."""
        f = flags if flags is not None else (RTU_QUERY_REFERENCE_WALK if reference_walk else 0)
        self._check(hip.rtu_occluded_rays_device(self._h, d_rays_ptr, n, f, d_occluded_ptr, stream))

    def render_frames_device(self, frames, d_ptr, stream=None):
        """Frames in flight: len(frames) frames of recipe W in one launch sequence, images consecutive at d_ptr."""
        arr = (RtuFrameDesc * len(frames))(*frames)
        self._check(hip.rtu_render_frames_device(self._h, arr, len(frames), d_ptr, stream))

    def pack_image_device(self, d_rgbz, n_pixels, d_z, d_rgb8, stream=None):
        """float4 image -> float z + Color24 pixels (the reference's RenderImage content), on the device."""
        self._check(hip.rtu_pack_image_device(self._h, d_rgbz, n_pixels, d_z, d_rgb8, stream))

    def minmax_z_device(self, d_rgbz, pixels_per_frame, n_frames, d_minmax, stream=None):
        """Per frame of a batch: keys of this shard's zmin / zmax as int64 pairs (all-reduce MIN over the shards gives the frame's)."""
        self._check(hip.rtu_minmax_z_device(self._h, d_rgbz, pixels_per_frame, n_frames, d_minmax, stream))

    def pack_output_device(self, d_rgbz, pixels_per_frame, n_frames, d_minmax, d_out4, stream=None):
        """float4 images -> 4 bytes per pixel {Color24, z-image byte}: the content of Result.png and ZBuffer.png."""
        self._check(hip.rtu_pack_output_device(self._h, d_rgbz, pixels_per_frame, n_frames, d_minmax, d_out4, stream))

    def frame_status(self):
        """Synchronise; raises RtuError(RTU_ERR_CAPACITY) if the frame must be rendered again."""
        self._check(hip.rtu_frame_status(self._h))

    TIMELINE_SLOTS = (["k_primary", "k_primary2c", "k_primary2"] +
                      ["%s(L%d)" % (k, L) for L in range(6) for k in ("k_trace", "k_trace2c", "k_trace2", "k_consume")] +
                      ["k_combine(L%d)" % L for L in range(6)])
    # when the tail kernel (k_tail) takes over from level Ls, its stamps are in the k_trace(L<Ls>) slot

    def render_timeline(self, frame, d_ptr):
        """One frame with in-kernel GPU-clock stamps: [(kernel, start_us, end_us)] in launch order."""
        n = 40
        slot, t0, t1 = (_I * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
        rc = hip.rtu_render_timeline(self._h, ctypes.byref(frame), d_ptr, n, slot, t0, t1)
        if rc < 0:
            self._check(rc)
        order = {name: i for i, name in enumerate(self.TIMELINE_SLOTS)}
        rows = [(self.TIMELINE_SLOTS[slot[i]], t0[i], t1[i]) for i in range(rc)]
        # launch order: combines run bottom-up after everything else
        return sorted(rows, key=lambda r: (r[0].startswith("k_combine"), -order[r[0]] if r[0].startswith("k_combine") else order[r[0]]))

    def timeline_exits(self, kernel):
        """Exit times (us after the kernel's first entry) of the wavefronts of `kernel` (a name of
        TIMELINE_SLOTS) in the frame last rendered by render_timeline."""
        import numpy as np
        buf = (ctypes.c_double * 8192)()
        rc = hip.rtu_timeline_exits(self._h, self.TIMELINE_SLOTS.index(kernel), 8192, buf)
        if rc < 0:
            self._check(rc)
        return np.array(buf[:rc])

    def mesh_info(self, mesh=0):
        """dict(faces, sah_depth, stack4, nodes4, nodes8) of an uploaded mesh."""
        o = (ctypes.c_uint32 * 5)()
        self._check(hip.rtu_mesh_info(self._h, mesh, o))
        return dict(zip(("faces", "sah_depth", "stack4", "nodes4", "nodes8"), list(o)))

    def light_lists(self):
        """[dict(light, cover, G, entries, longest)]: the occluder lists of shadow rays built at upload."""
        out, i = [], 0
        while True:
            o = (ctypes.c_uint32 * 5)()
            if hip.rtu_light_list_info(self._h, i, o) != 0:
                return out
            out.append(dict(zip(("light", "cover", "G", "entries", "longest"), list(o))))
            i += 1

    def frame_counts(self):
        """(frames per level [6], rays deferred to stage 2 per phase [7]) of the most recent frame."""
        fr, de = (ctypes.c_uint32 * 6)(), (ctypes.c_uint32 * 7)()
        self._check(hip.rtu_frame_counts(self._h, fr, de))
        return list(fr), list(de)

    def time_render(self, frame, d_ptr, stream, iters):
        ms = ctypes.c_float(0)
        self._check(hip.rtu_time_render(self._h, ctypes.byref(frame), d_ptr, stream, iters, ctypes.byref(ms)))
        return ms.value

    def touched(self, textured=False):
        """Touched-bytes mode (frame.collect_stats == 2): {kernel slot name: counters + 'bytes'} of the launches of the most
        recent launch sequence that touched anything."""
        arr = (RtuTouched * KERNEL_SLOTS)()
        n = hip.rtu_get_touched(self._h, arr, KERNEL_SLOTS)
        if n < 0:
            self._check(n)
        nl = (ctypes.c_uint32 * KERNEL_SLOTS)()
        hip.rtu_get_touched_launches(self._h, nl, KERNEL_SLOTS)
        out = {}
        for k in range(n):
            d = arr[k].as_dict()
            if any(d.values()):
                d["bytes"] = int(hip.rtu_touched_bytes(ctypes.byref(arr[k]), 1 if textured else 0))
                d["launches"] = int(nl[k])  # of this slot's kernel since the counters were zeroed (a sampled frame is many launch sequences)
                out[hip.rtu_kernel_slot_name(k).decode()] = d
        return out

    def probe_kernel(self, slot_name):
        """Bracket every launch of that kernel slot ('k_trace2(L0)', ...; None: stop) with HIP events on its stream."""
        slot = -1
        if slot_name is not None:
            names = [hip.rtu_kernel_slot_name(k).decode() for k in range(KERNEL_SLOTS)]
            slot = names.index(slot_name)
        self._check(hip.rtu_probe_kernel(self._h, slot))

    def probe_read(self):
        """(summed milliseconds, launches measured) since the last read; synchronises."""
        ms, n = ctypes.c_float(0), _I(0)
        self._check(hip.rtu_probe_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def stats(self):
        st = RtuStats()
        self._check(hip.rtu_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            hip.rtu_destroy_context(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_rows(frame):
    return hip.rtu_shard_rows(ctypes.byref(frame))


def shard_global_rows(frame):
    """Global row index of every local row of this shard."""
    import numpy as np
    n = shard_rows(frame)
    return np.array([hip.rtu_shard_global_row(ctypes.byref(frame), i) for i in range(n)], dtype=np.int64)


def assemble(shards, frames, height):
    """De-interleave per-shard compact buffers into one [H, W, 4] image."""
    import numpy as np
    w = frames[0].width
    out = np.empty((height, w, 4), np.float32)
    for buf, fr in zip(shards, frames):
        rows = shard_global_rows(fr)
        out[rows] = buf[:len(rows)]
    return out


class Image:
    """RenderImage mirror (RtuImage*): Color24 pixels, float z-buffer, z-image."""

    def __init__(self, width, height):
        self._h = host.rtu_image_create(width, height)
        self.width, self.height = width, height

    def fill(self, rgbz, row0=0):
        import numpy as np
        a = np.ascontiguousarray(rgbz, dtype=np.float32)
        host.rtu_image_from_rgbz(self._h, a.ctypes.data, row0, a.shape[0])

    def compute_zimage(self):
        host.rtu_image_compute_zimg(self._h)

    def pixels(self):
        import numpy as np
        p = host.rtu_image_pixels(self._h)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)),
                                     (self.height, self.width, 3)).copy()

    def zbuffer(self):
        import numpy as np
        p = host.rtu_image_zbuffer(self._h)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), (self.height, self.width)).copy()

    def zimage(self):
        import numpy as np
        p = host.rtu_image_zimage(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (self.height, self.width)).copy()

    def sample_count(self):
        import numpy as np
        p = host.rtu_image_sample_count(self._h)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (self.height, self.width)).copy()

    def fill_sample_count(self, counts, row0=0):
        import numpy as np
        a = np.ascontiguousarray(counts, dtype=np.uint8)
        host.rtu_image_fill_sample_count(self._h, a.ctypes.data, row0, a.shape[0])

    def compute_sample_count_image(self):
        """ComputeSampleCountImage: returns smax."""
        return host.rtu_image_compute_sample_count_img(self._h)

    def sample_count_image(self):
        import numpy as np
        p = host.rtu_image_sample_count_image(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (self.height, self.width)).copy()

    def save_sample_count(self, path):
        if host.rtu_image_save_sample_count_png(self._h, path.encode()) != 0:
            raise RtuError(RTU_ERR_ARG, "cannot write " + path)

    def save(self, result_png=None, zbuffer_png=None):
        if result_png and host.rtu_image_save_png(self._h, result_png.encode()) != 0:
            raise RtuError(RTU_ERR_ARG, "cannot write " + result_png)
        if zbuffer_png and host.rtu_image_save_zpng(self._h, zbuffer_png.encode()) != 0:
            raise RtuError(RTU_ERR_ARG, "cannot write " + zbuffer_png)

    def close(self):
        if self._h:
            host.rtu_image_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
