"""Host-side mirror of the reference's interface for the hot path, over the C ABI of include/nrc_hpm.h.

Same class / method names and argument meaning as the reference (so parity tests read like reference call sites):
  AppConfig             include/engine/AppConfig.hpp:9-66, src/AppConfig.cpp:154-182 (17 positional CLI args)
  NeuralRadianceCache   include/engine/graphics/NeuralRadianceCache.hpp:13-32
  NrcHpmRenderer        include/engine/graphics/renderer/NrcHpmRenderer.hpp:16-41
  McHpmRenderer         include/engine/graphics/renderer/McHpmRenderer.hpp:16-31
Errors raise RuntimeError("SkyRenderer ERROR: ...") like Log::Error(msg, true) (src/Log.cpp:16-20).

PyTorch is plumbing only (device memory, current stream, torch.distributed); all arithmetic runs in libnrc_hpm.so.
There is no CPU fallback: loading fails loudly if the HIP library is missing.
"""
import ctypes as C
import functools
import inspect
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NRC_HPM_LIB: tooling override (tools/loop_profile.py loads an instrumented build)
LIB_PATH = os.environ.get("NRC_HPM_LIB") or os.path.join(_HERE, "lib", "libnrc_hpm.so")

NRC_FIX_Q1_TRAIN_Y_DIST = 1
NRC_FIX_Q2_TRAIN_RAY_LEN = 2
NRC_NONFINITE_PROPAGATE = 0      # include/nrc_hpm.h, nrc_cache_set_nonfinite_policy
NRC_NONFINITE_SKIP = 1


class NrcConfig(C.Structure):
    _fields_ = [
        ("loss_fn", C.c_char * 32), ("optimizer", C.c_char * 32),
        ("learning_rate", C.c_float), ("ema_decay", C.c_float),
        ("pos_id", C.c_uint32), ("dir_id", C.c_uint32), ("nn_width", C.c_uint32), ("nn_depth", C.c_uint32),
        ("log2_infer_batch_size", C.c_uint32), ("log2_train_batch_size", C.c_uint32), ("train_batch_count", C.c_uint32),
        ("scene_id", C.c_uint32), ("train_ring_buf_size", C.c_float), ("train_spp", C.c_uint32),
        ("primary_ray_length", C.c_uint32), ("primary_ray_prob", C.c_float), ("train_ray_length", C.c_uint32),
        ("seed", C.c_uint32), ("compat_fix", C.c_uint32), ("hashgrid_log2_size", C.c_uint32),
        ("self_train", C.c_uint32),      # since nrc_version() 0.3 (include/nrc_hpm.h: self-training)
    ]


class NrcScene(C.Structure):
    _fields_ = [
        ("density", C.c_void_p), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32),
        ("size", C.c_float * 3), ("density_factor", C.c_float), ("g", C.c_float),
        ("dir_light_dir", C.c_float * 3), ("dir_light_strength", C.c_float),
        ("point_light_pos", C.c_float * 3), ("point_light_strength", C.c_float),
        ("point_light_color", C.c_float * 3), ("env_strength", C.c_float),
        ("env", C.c_void_p), ("env_w", C.c_uint32), ("env_h", C.c_uint32),
    ]


class NrcCamera(C.Structure):
    _fields_ = [("inv_proj_view", C.c_float * 16), ("pos", C.c_float * 3)]


class NrcTile(C.Structure):
    _fields_ = [("x_offset", C.c_uint32), ("x_stride", C.c_uint32), ("global_w", C.c_uint32), ("global_h", C.c_uint32),
                ("x_block", C.c_uint32)]


GRAD_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)
ALLREDUCE_F64_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p)
ALLGATHER_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

# every symbol include/nrc_hpm.h declares (tests/test_abi.py checks the built library exports all of them)
ABI_SYMBOLS = [
    "nrc_last_error", "nrc_version", "nrc_config_default",
    "nrc_cache_create", "nrc_cache_init", "nrc_cache_init_events", "nrc_cache_infer_and_train", "nrc_cache_destroy", "nrc_cache_get_loss",
    "nrc_cache_get_loss_blocking", "nrc_cache_get_loss_async", "nrc_cache_comm_info", "nrc_cache_comm_time_exchange", "nrc_renderer_release_frame", "nrc_renderer_is_blending", "nrc_mc_renderer_is_blending",
    "nrc_renderer_set_full_vertex_images", "nrc_renderer_vertex_image_bytes", "nrc_renderer_set_empty_skip", "nrc_mc_renderer_set_empty_skip",
    "nrc_cache_set_collective_hooks", "nrc_renderer_gather_frame", "nrc_renderer_export_exr_gathered", "nrc_compare_images_sharded",
    "nrc_renderer_set_cost_order", "nrc_renderer_set_schedule", "nrc_renderer_get_schedule", "nrc_renderer_schedule_source", "nrc_renderer_schedule_key",
    "nrc_schedule_cache_load", "nrc_schedule_cache_save", "nrc_schedule_cache_clear", "nrc_renderer_tile_order", "nrc_mc_renderer_set_cost_order", "nrc_renderer_set_hot_tiles", "nrc_renderer_hot_tiles",
    "nrc_cache_get_infer_batch_count", "nrc_cache_get_train_batch_count", "nrc_cache_get_infer_batch_size",
    "nrc_cache_get_train_batch_size", "nrc_cache_infer", "nrc_cache_backward", "nrc_cache_optimizer_step",
    "nrc_cache_grad_ptr", "nrc_cache_param_count", "nrc_cache_loss_ptr", "nrc_cache_set_loss_norm_factor",
    "nrc_comm_unique_id", "nrc_cache_comm_init", "nrc_cache_comm_sparse", "nrc_cache_grid_list_capacity",
    "nrc_cache_set_exchange_dtype", "nrc_cache_get_exchange_dtype",
    "nrc_cache_set_nonfinite_policy", "nrc_cache_get_nonfinite_policy", "nrc_cache_get_skipped_steps",
    "nrc_cache_grid_grad_pack", "nrc_cache_grid_grad_apply",
    "nrc_cache_set_stream", "nrc_cache_set_grad_hook", "nrc_cache_get_params", "nrc_cache_set_params",
    "nrc_cache_get_step", "nrc_cache_set_step", "nrc_cache_param_count_tcnn", "nrc_cache_get_params_tcnn", "nrc_cache_set_params_tcnn",
    "nrc_cache_save_checkpoint", "nrc_cache_load_checkpoint", "nrc_cache_comm_status", "nrc_cache_set_comm_timeout_ms",
    "nrc_renderer_create", "nrc_renderer_render", "nrc_renderer_render_frames", "nrc_renderer_set_stage_events", "nrc_renderer_set_camera", "nrc_renderer_set_blend",
    "nrc_renderer_set_scene_params", "nrc_mc_renderer_set_scene_params",
    "nrc_renderer_set_volume", "nrc_mc_renderer_set_volume", "nrc_renderer_volume_buffer", "nrc_mc_renderer_volume_buffer",
    "nrc_renderer_set_volume_bricks", "nrc_mc_renderer_set_volume_bricks",
    "nrc_renderer_set_volume_keys", "nrc_mc_renderer_set_volume_keys", "nrc_renderer_volume_key_count", "nrc_mc_renderer_volume_key_count",
    "nrc_renderer_set_volume_key_bricks", "nrc_mc_renderer_set_volume_key_bricks", "nrc_renderer_volume_key_bytes", "nrc_mc_renderer_volume_key_bytes",
    "nrc_renderer_set_volume_time", "nrc_mc_renderer_set_volume_time", "nrc_renderer_render_path_timed", "nrc_mc_renderer_render_path_timed",
    "nrc_renderer_render_path", "nrc_mc_renderer_render_path", "nrc_renderer_tile_mask", "nrc_mc_renderer_tile_mask",
    "nrc_renderer_tile_far", "nrc_mc_renderer_tile_far", "nrc_renderer_cut_fetches",
    "nrc_renderer_view_aov", "nrc_mc_renderer_view_aov", "nrc_renderer_set_path_aov_target", "nrc_mc_renderer_set_path_aov_target",
    "nrc_renderer_export_exr_aov", "nrc_mc_renderer_export_exr_aov", "nrc_test_view_aov_host",
    "nrc_renderer_ray_aov", "nrc_mc_renderer_ray_aov", "nrc_renderer_view_aov_to_depth", "nrc_mc_renderer_view_aov_to_depth",
    "nrc_renderer_ortho_aov", "nrc_mc_renderer_ortho_aov", "nrc_renderer_set_path_aov_depths", "nrc_mc_renderer_set_path_aov_depths",
    "nrc_camera_rays", "nrc_ortho_rays", "nrc_test_ray_aov_host",
    "nrc_renderer_deep_ray_aov", "nrc_mc_renderer_deep_ray_aov", "nrc_renderer_deep_view_aov", "nrc_mc_renderer_deep_view_aov",
    "nrc_renderer_deep_ortho_aov", "nrc_mc_renderer_deep_ortho_aov", "nrc_test_deep_ray_aov_host",
    "nrc_denoise_params_default", "nrc_denoise_scratch_bytes", "nrc_denoise", "nrc_test_denoise_host",
    "nrc_renderer_denoised_frame", "nrc_mc_renderer_denoised_frame", "nrc_renderer_set_path_denoise_target", "nrc_mc_renderer_set_path_denoise_target",
    "nrc_renderer_export_exr_denoised", "nrc_mc_renderer_export_exr_denoised",
    "nrc_reproject_params_default", "nrc_reproject", "nrc_test_reproject_host",
    "nrc_renderer_set_path_reproject_target", "nrc_mc_renderer_set_path_reproject_target",
    "nrc_renderer_set_show_nrc", "nrc_renderer_set_frame_random", "nrc_renderer_framebuffer", "nrc_renderer_framebuffer_on",
    "nrc_renderer_export_exr",
    "nrc_renderer_frame_time_ms", "nrc_renderer_stage_stats", "nrc_renderer_frame_timeline", "nrc_set_wave_priority_raise", "nrc_renderer_destroy", "nrc_renderer_buffer", "nrc_renderer_count_fetches", "nrc_renderer_masked_fetches",
    "nrc_renderer_train_grid",
    "nrc_mc_renderer_create", "nrc_mc_renderer_render", "nrc_mc_renderer_set_camera", "nrc_mc_renderer_set_blend",
    "nrc_mc_renderer_set_frame_random", "nrc_mc_renderer_framebuffer", "nrc_mc_renderer_export_exr",
    "nrc_mc_renderer_frame_time_ms", "nrc_mc_renderer_count_fetches", "nrc_mc_renderer_destroy",
    "nrc_compare_images", "nrc_test_math", "nrc_test_rng", "nrc_test_flight_select", "nrc_debug_check_guards", "nrc_debug_live_allocations", "nrc_image_create", "nrc_image_destroy",
]

_lib = None


def set_wave_priority_raise(on=True):
    """nrc_set_wave_priority_raise: 1 (default) every kernel of the library at s_setprio 3, 0 at the hardware default (a process whose foreign
    kernels -- torch's NCCL all-reduce, fills, copies -- run beside the renderer)"""
    _check(load_library().nrc_set_wave_priority_raise(C.c_int(int(bool(on)))))


def build_id():
    """the hash of sources + compiler + flags the loaded library was built from (csrc/Makefile: NRC_BUILD_ID, the tail of nrc_version())"""
    v = load_library().nrc_version().decode()
    return v.rsplit("build ", 1)[1] if "build " in v else "unknown (a library older than the build id, loaded through NRC_HPM_LIB)"


def load_library():
    """dlopen libnrc_hpm.so (built by __graft_entry__.build() / csrc/Makefile).  No fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("SkyRenderer ERROR: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the NRC path)" % LIB_PATH)
    # ONE HIP runtime per process: torch bundles its own libamdhip64.so (soname libamdhip64.so.7).  Import torch first so
    # that libnrc_hpm.so's NEEDED libamdhip64.so.7 binds to the copy torch already loaded -- streams and device pointers
    # handed over from torch are only meaningful inside the same runtime instance.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.nrc_last_error.restype = C.c_char_p
    L.nrc_version.restype = C.c_char_p
    L.nrc_cache_get_loss.restype = C.c_float
    L.nrc_cache_get_loss_blocking.restype = C.c_float
    L.nrc_cache_get_infer_batch_count.restype = C.c_size_t
    L.nrc_cache_get_train_batch_count.restype = C.c_size_t
    L.nrc_cache_get_infer_batch_size.restype = C.c_uint32
    L.nrc_cache_grid_list_capacity.restype = C.c_size_t
    L.nrc_cache_get_train_batch_size.restype = C.c_uint32
    L.nrc_cache_grad_ptr.restype = C.c_void_p
    L.nrc_cache_loss_ptr.restype = C.c_void_p
    L.nrc_cache_param_count.restype = C.c_uint32
    L.nrc_cache_param_count_tcnn.restype = C.c_uint32
    L.nrc_cache_param_count_tcnn.argtypes = [C.c_void_p]
    L.nrc_renderer_framebuffer.restype = C.c_void_p
    L.nrc_renderer_framebuffer_on.restype = C.c_void_p
    L.nrc_renderer_buffer.restype = C.c_void_p
    L.nrc_renderer_frame_time_ms.restype = C.c_float
    L.nrc_renderer_vertex_image_bytes.restype = C.c_size_t
    L.nrc_renderer_vertex_image_bytes.argtypes = [C.c_void_p]
    L.nrc_renderer_tile_order.restype = C.c_size_t
    L.nrc_renderer_tile_order.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.nrc_mc_renderer_framebuffer.restype = C.c_void_p
    for name in ("nrc_renderer_set_volume", "nrc_mc_renderer_set_volume"):
        if hasattr(L, name):      # (an older build loaded through NRC_HPM_LIB has no volume swap)
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    for name in ("nrc_renderer_set_volume_bricks", "nrc_mc_renderer_set_volume_bricks"):
        if hasattr(L, name):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
    for name in ("nrc_renderer_volume_buffer", "nrc_mc_renderer_volume_buffer"):
        if hasattr(L, name):
            getattr(L, name).restype = C.c_void_p
            getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    for name in ("nrc_renderer_tile_mask", "nrc_mc_renderer_tile_mask", "nrc_renderer_tile_far", "nrc_mc_renderer_tile_far"):
        if hasattr(L, name):      # (an older build loaded through NRC_HPM_LIB has no camera paths)
            getattr(L, name).restype = C.c_size_t
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    if hasattr(L, "nrc_renderer_render_path"):
        L.nrc_renderer_render_path.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
        L.nrc_mc_renderer_render_path.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(L, "nrc_renderer_set_volume_keys"):      # (an older build loaded through NRC_HPM_LIB has no volume keys)
        for name in ("nrc_renderer_set_volume_keys", "nrc_mc_renderer_set_volume_keys"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
        for name in ("nrc_renderer_volume_key_count", "nrc_mc_renderer_volume_key_count"):
            getattr(L, name).restype = C.c_uint32
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("nrc_renderer_set_volume_time", "nrc_mc_renderer_set_volume_time"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_float]
        L.nrc_renderer_render_path_timed.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
        L.nrc_mc_renderer_render_path_timed.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(L, "nrc_renderer_set_volume_key_bricks"):      # (an older build loaded through NRC_HPM_LIB has no brick keys)
        for name in ("nrc_renderer_set_volume_key_bricks", "nrc_mc_renderer_set_volume_key_bricks"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int]
        for name in ("nrc_renderer_volume_key_bytes", "nrc_mc_renderer_volume_key_bytes"):
            getattr(L, name).restype = C.c_size_t
            getattr(L, name).argtypes = [C.c_void_p]
    if hasattr(L, "nrc_renderer_view_aov"):      # (an older build loaded through NRC_HPM_LIB has no view AOV)
        for name in ("nrc_renderer_view_aov", "nrc_mc_renderer_view_aov"):
            getattr(L, name).restype = C.c_void_p
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("nrc_renderer_set_path_aov_target", "nrc_mc_renderer_set_path_aov_target"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        for name in ("nrc_renderer_export_exr_aov", "nrc_mc_renderer_export_exr_aov"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_char_p]
        L.nrc_test_view_aov_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(L, "nrc_renderer_ray_aov"):      # (an older build loaded through NRC_HPM_LIB has no ray AOV)
        for name in ("nrc_renderer_ray_aov", "nrc_mc_renderer_ray_aov"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        for name in ("nrc_renderer_view_aov_to_depth", "nrc_mc_renderer_view_aov_to_depth"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("nrc_renderer_ortho_aov", "nrc_mc_renderer_ortho_aov"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        for name in ("nrc_renderer_set_path_aov_depths", "nrc_mc_renderer_set_path_aov_depths"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.nrc_camera_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.nrc_ortho_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.nrc_test_ray_aov_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    if hasattr(L, "nrc_renderer_deep_ray_aov"):      # (an older build loaded through NRC_HPM_LIB has no deep AOV)
        for name in ("nrc_renderer_deep_ray_aov", "nrc_mc_renderer_deep_ray_aov"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("nrc_renderer_deep_view_aov", "nrc_mc_renderer_deep_view_aov"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("nrc_renderer_deep_ortho_aov", "nrc_mc_renderer_deep_ortho_aov"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nrc_test_deep_ray_aov_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "nrc_denoise"):      # (an older build loaded through NRC_HPM_LIB has no denoise filter)
        L.nrc_denoise_params_default.restype = None
        L.nrc_denoise_params_default.argtypes = [C.c_void_p]
        L.nrc_denoise_scratch_bytes.restype = C.c_size_t
        L.nrc_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        L.nrc_denoise.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nrc_test_denoise_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        for name in ("nrc_renderer_denoised_frame", "nrc_mc_renderer_denoised_frame"):
            getattr(L, name).restype = C.c_void_p
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        for name in ("nrc_renderer_set_path_denoise_target", "nrc_mc_renderer_set_path_denoise_target"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        for name in ("nrc_renderer_export_exr_denoised", "nrc_mc_renderer_export_exr_denoised"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    if hasattr(L, "nrc_reproject"):      # (an older build loaded through NRC_HPM_LIB has no reprojection)
        L.nrc_reproject_params_default.restype = None
        L.nrc_reproject_params_default.argtypes = [C.c_void_p]
        L.nrc_reproject.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nrc_test_reproject_host.argtypes = L.nrc_reproject.argtypes[:-1]
        for name in ("nrc_renderer_set_path_reproject_target", "nrc_mc_renderer_set_path_reproject_target"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.nrc_mc_renderer_frame_time_ms.restype = C.c_float
    if hasattr(L, "nrc_test_flight_select"):      # (an older build loaded through NRC_HPM_LIB has no such hook)
        L.nrc_test_flight_select.argtypes = [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("nrc_cache_get_loss", "nrc_cache_get_loss_blocking", "nrc_renderer_is_blending", "nrc_mc_renderer_is_blending",
                 "nrc_cache_get_infer_batch_count", "nrc_cache_get_train_batch_count",
                 "nrc_cache_get_infer_batch_size", "nrc_cache_get_train_batch_size", "nrc_cache_grad_ptr",
                 "nrc_cache_loss_ptr", "nrc_cache_param_count", "nrc_renderer_framebuffer", "nrc_mc_renderer_framebuffer",
                 "nrc_mc_renderer_frame_time_ms"):
        getattr(L, name).argtypes = [C.c_void_p]
    _lib = L
    # schedules the tuner settled on in earlier processes (include/nrc_hpm.h, nrc_schedule_cache_load): the package's own table -- this pool's
    # MI355X, the BASELINE presets -- and the host's (NRC_SCHEDULE_CACHE=<file>; "" = none of either)
    if hasattr(L, "nrc_schedule_cache_load"):
        L.nrc_renderer_schedule_source.restype = C.c_char_p
        L.nrc_renderer_schedule_key.restype = C.c_char_p
        user = os.environ.get("NRC_SCHEDULE_CACHE")
        for path in ([] if user == "" else [os.path.join(_HERE, "schedules.txt")] + ([user] if user else [])):
            if os.path.exists(path):
                L.nrc_schedule_cache_load(path.encode(), None)
    return L


def load_schedule_cache(path):
    """nrc_schedule_cache_load: merge a file of tuned schedules into the process-wide table; returns the number of entries read"""
    n = C.c_int(0)
    _check(load_library().nrc_schedule_cache_load(path.encode(), C.byref(n)))
    return n.value


def clear_schedule_cache():
    _check(load_library().nrc_schedule_cache_clear())


def save_schedule_cache(path):
    """nrc_schedule_cache_save: write the process-wide table (what the tuners of this process settled on + what was loaded)"""
    n = C.c_int(0)
    _check(load_library().nrc_schedule_cache_save(path.encode(), C.byref(n)))
    return n.value


class CommError(RuntimeError):
    """NRC_ERR_COMM: a collective failed or a peer did not answer within the communicator's deadline; the communicator is aborted"""


def _check(status):
    if status != 0:
        msg = load_library().nrc_last_error().decode() or "SkyRenderer ERROR: status %d" % status
        raise (CommError if status == -4 else RuntimeError)(msg)


def _vp(x):
    return C.c_void_p(int(x) if x is not None else 0)


def _dev_ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


# ------------------------------------------------------------------------------------------------------------------
class AppConfig:
    """en::AppConfig.  AppConfig(argv) takes the reference's 18-entry argv (program name + 17 args,
    src/AppConfig.cpp:154-182); AppConfig() gives the defaults of src/main.cu:432-439 with the north-star
    encoding (posID 3 Frequency, dirID 0 OneBlob)."""

    def __init__(self, argv=None, **overrides):
        c = NrcConfig()
        load_library().nrc_config_default(C.byref(c))
        if argv is not None:
            if len(argv) != 18:
                raise RuntimeError("SkyRenderer ERROR: Argument count does not match requirements for AppConfig")
            a = [str(x) for x in argv[1:]]
            c.loss_fn, c.optimizer = a[0].encode(), a[1].encode()
            c.learning_rate, c.ema_decay = float(a[2]), float(a[3])
            c.pos_id, c.dir_id = int(a[4]), int(a[5])
            c.nn_width, c.nn_depth = int(a[6]), int(a[7])
            c.log2_infer_batch_size, c.log2_train_batch_size, c.train_batch_count = int(a[8]), int(a[9]), int(a[10])
            c.scene_id = int(a[11])
            c.train_ring_buf_size, c.train_spp = float(a[12]), int(a[13])
            c.primary_ray_length, c.primary_ray_prob, c.train_ray_length = int(a[14]), float(a[15]), int(a[16])
        for k, v in overrides.items():
            if not hasattr(c, k):
                raise AttributeError(k)
            setattr(c, k, v.encode() if isinstance(v, str) else v)
        self.c = c

    def __getattr__(self, k):
        v = getattr(self.__dict__["c"], k)
        return v.decode() if isinstance(v, bytes) else v

    def GetName(self):      # src/AppConfig.cpp:184-205 (std::to_string formatting)
        c = self.c
        f = "%.6f"
        parts = [c.loss_fn.decode(), c.optimizer.decode(), f % c.learning_rate, f % c.ema_decay, c.pos_id, c.dir_id,
                 c.nn_width, c.nn_depth, c.log2_infer_batch_size, c.log2_train_batch_size, c.train_batch_count,
                 c.scene_id, f % c.train_ring_buf_size, c.train_spp, c.primary_ray_length, f % c.primary_ray_prob,
                 c.train_ray_length]
        return "_".join(str(p) for p in parts)


def make_c_scene(scene):
    """dict from nrc_hpm_renderer_amd.scene.make_scene -> nrc_scene (host pointers; keeps the arrays alive)."""
    s = NrcScene()
    dens = np.ascontiguousarray(scene["density"], np.uint8)
    env = np.ascontiguousarray(scene["env"], np.float32)
    s.density = dens.ctypes.data
    s.nx, s.ny, s.nz = scene["dims"]
    s.size[:] = [float(x) for x in scene["size"]]
    s.density_factor = scene["density_factor"]
    s.g = scene["g"]
    s.dir_light_dir[:] = [float(x) for x in scene["dir_light_dir"]]
    s.dir_light_strength = scene["dir_light_strength"]
    s.point_light_pos[:] = [float(x) for x in scene["point_light_pos"]]
    s.point_light_strength = scene["point_light_strength"]
    s.point_light_color[:] = [float(x) for x in scene["point_light_color"]]
    s.env_strength = scene["env_strength"]
    s.env = env.ctypes.data
    s.env_h, s.env_w = env.shape[0], env.shape[1]
    s._keep = (dens, env)
    return s


def make_c_camera(cam):
    c = NrcCamera()
    c.inv_proj_view[:] = [float(x) for x in np.asarray(cam["inv_proj_view"], np.float32).reshape(16)]
    c.pos[:] = [float(x) for x in cam["pos"]]
    return c


def _wrap_device(ptr, nbytes, dtype, shape):
    """torch view over a device pointer owned by the library (no copy)."""
    import torch

    class _Arr:
        pass

    a = _Arr()
    a.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    t = torch.as_tensor(a, device="cuda")
    return t.view(dtype).view(*shape)


VOLUME_U8, VOLUME_F32 = 0, 1      # NRC_VOLUME_U8 / NRC_VOLUME_F32
VOLUME_BUF = dict(density=0, occ_bits=1, boxes=2)


def _brick_list(who, origins, bricks):
    """a brick list of SetVolumeBricks / SetVolumeKeyBricks (`who`, for the error text): origins int32 [n][3] and bricks uint8 or float32
    [n][8][8][8] ([dz][dy][dx]), both C-contiguous numpy arrays (host memory: the call copies them and waits for the copy) or both
    contiguous CUDA torch tensors (read on the renderer's stream; the call does not wait).  Returns what the library call takes: the two
    pointers (None for an empty list), n, the format and on_device."""
    if isinstance(origins, np.ndarray) and isinstance(bricks, np.ndarray):
        if origins.dtype != np.int32 or origins.ndim != 2 or origins.shape[1] != 3 or not origins.flags.c_contiguous \
                or bricks.dtype not in (np.uint8, np.float32) or bricks.shape != (origins.shape[0], 8, 8, 8) or not bricks.flags.c_contiguous:
            raise RuntimeError("SkyRenderer ERROR: %s takes C-contiguous numpy arrays, origins int32 [n][3] and bricks uint8 or "
                               "float32 [n][8][8][8] (got %s %s and %s %s)" % (who, origins.dtype, origins.shape, bricks.dtype, bricks.shape))
        on_device, f32, ptr = 0, bricks.dtype == np.float32, lambda a: C.c_void_p(a.ctypes.data)
    else:
        import torch
        ok = isinstance(origins, torch.Tensor) and isinstance(bricks, torch.Tensor) and origins.is_cuda and bricks.is_cuda \
            and origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 3 and origins.is_contiguous() \
            and bricks.dtype in (torch.uint8, torch.float32) and tuple(bricks.shape) == (origins.shape[0], 8, 8, 8) and bricks.is_contiguous()
        if not ok:
            raise RuntimeError("SkyRenderer ERROR: %s takes contiguous CUDA tensors, origins int32 [n][3] and bricks uint8 or float32 "
                               "[n][8][8][8], or two numpy arrays of those types" % who)
        on_device, f32, ptr = 1, bricks.dtype == torch.float32, _dev_ptr
    n = origins.shape[0]
    return ptr(origins) if n else None, ptr(bricks) if n else None, n, VOLUME_F32 if f32 else VOLUME_U8, on_device


def _set_volume_key_bricks(fn, h, counts, origins, bricks):
    """SetVolumeKeyBricks of both renderers: counts, the bricks of every key (a sequence of ints or an integer numpy array, always host
    memory), and the keys' lists concatenated in key order -- origins int32 [sum(counts)][3] and bricks uint8 or float32 [sum(counts)][8][8][8],
    validated like SetVolumeBricks' (two C-contiguous numpy arrays or two contiguous CUDA tensors).  counts None or empty drops the sequence."""
    if counts is None or len(counts) == 0:
        _check(fn(h, None, None, None, 0, VOLUME_U8, 0))
        return
    counts64 = np.asarray(counts)
    if counts64.ndim != 1 or counts64.dtype.kind not in "iu" or (counts64 < 0).any() or (counts64 > 0xffffffff).any():
        raise RuntimeError("SkyRenderer ERROR: SetVolumeKeyBricks takes counts as a sequence of non-negative integers, one per key (got %r)" % (counts,))
    key_counts = np.ascontiguousarray(counts64, np.uint32)
    total = int(counts64.astype(np.uint64).sum())
    p_origins, p_bricks, n, fmt, on_device = _brick_list("SetVolumeKeyBricks", origins, bricks)
    if n != total:
        raise RuntimeError("SkyRenderer ERROR: SetVolumeKeyBricks: counts sum to %d bricks, origins and bricks hold %d" % (total, n))
    _check(fn(h, C.c_void_p(key_counts.ctypes.data), p_origins, p_bricks, key_counts.size, fmt, on_device))


def _render_path(call, width, height, cameras, framesPerCamera, frameRandoms, out, times=None):
    """RenderPath of both renderers: cameras is a sequence of scene.make_camera dicts, frameRandoms None or [len(cameras) * framesPerCamera][4],
    out None (a new tensor is returned) or a contiguous float32 CUDA tensor [len(cameras)][height][width][4], or False (no images: the last
    view stays in GetImage()), times None or len(cameras) times into the volume keys.  call(n, cameras pointer, frames per camera, randoms
    pointer, images pointer[, times pointer]) makes the library call."""
    import torch
    cams = list(cameras)
    n, fpc = len(cams), int(framesPerCamera)
    if fpc < 0:
        raise ValueError("RenderPath: framesPerCamera must not be negative")
    t = None
    if times is not None:
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        if t.size != n:
            raise ValueError("RenderPath: %d times for %d views" % (t.size, n))
    arr = (NrcCamera * max(n, 1))(*[make_c_camera(c) for c in cams])
    r = None
    if frameRandoms is not None:
        r = np.ascontiguousarray(frameRandoms, np.float32).reshape(-1)
        if r.size != n * fpc * 4:
            raise ValueError("RenderPath: frameRandoms holds %d floats, %d views x %d frames need %d" % (r.size, n, fpc, n * fpc * 4))
    shape = (n, height, width, 4)
    if out is None:
        out = torch.empty(shape, device="cuda", dtype=torch.float32)
    elif out is not False:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("RenderPath: out must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
    args = (C.c_uint32(n), C.cast(arr, C.c_void_p), C.c_uint32(fpc), C.c_void_p(r.ctypes.data) if r is not None else None,
            _dev_ptr(out) if out is not False and n else None)
    _check(call(*args) if t is None else call(*args, C.c_void_p(t.ctypes.data)))
    return None if out is False else out


def _check_device_floats(what, t, shape):
    """a contiguous float32 CUDA tensor of `shape`, as RenderPath checks aov_out"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous float32 CUDA tensor of shape %s" % (what, tuple(shape)))
    return t


def _aov_out(what, out, shape):
    """`out` checked, or a new tensor of `shape`"""
    import torch
    if out is None:
        return torch.empty(tuple(shape), device="cuda", dtype=torch.float32)
    return _check_device_floats(what + ": out", out, shape)


def _deep_levels_arg(levels):
    """(contiguous float32 array, K) of the deep AOV's levels; the library checks their order and range"""
    lv = np.ascontiguousarray(np.asarray(levels, np.float32).reshape(-1))
    if lv.size == 0 or lv.size > 32:
        raise ValueError("deep AOV: 1 .. 32 levels, not %d" % lv.size)
    return lv, int(lv.size)


def _deep_flat(what, flat, shape):
    """the optional flat result: None, True (a new tensor) or the caller's tensor, checked"""
    if flat is None or flat is False:
        return None
    return _aov_out(what + ": flat", None if flat is True else flat, shape)


class NrcDenoiseParams(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("sigma_alpha", C.c_float), ("sigma_depth", C.c_float), ("sigma_color", C.c_float),
                ("color_decay", C.c_float)]


def make_c_denoise_params(params=None):
    """nrc_denoise_params: the library's defaults (nrc_denoise_params_default) overridden by `params` -- None, a dict with any of passes,
    sigma_alpha, sigma_depth, sigma_color, color_decay (scene.denoise_params), or an NrcDenoiseParams.  The library checks the values."""
    if isinstance(params, NrcDenoiseParams):
        return params
    p = NrcDenoiseParams()
    load_library().nrc_denoise_params_default(C.byref(p))
    for k, v in (params or {}).items():
        if k not in ("passes", "sigma_alpha", "sigma_depth", "sigma_color", "color_decay"):
            raise ValueError("denoise parameters: unknown key %r" % (k,))
        setattr(p, k, int(v) if k == "passes" else float(v))
    return p


def Denoise(rgba, aov, params=None, out=None):
    """nrc_denoise: the edge-avoiding a-trous filter (include/nrc_hpm.h, "Denoise") over whole images -- what a caller with a gathered frame
    uses.  rgba and aov: contiguous float32 CUDA tensors [h][w][4] (a framebuffer and the view AOV of the same view); params as for
    make_c_denoise_params.  Returns the filtered image [h][w][4] (`out`, or a new tensor; never one of the inputs).  Enqueued on torch's
    current stream; no host wait."""
    import torch
    if not isinstance(rgba, torch.Tensor) or rgba.dim() != 3:
        raise ValueError("Denoise: rgba must be a contiguous float32 CUDA tensor of shape (h, w, 4)")
    shape = (int(rgba.shape[0]), int(rgba.shape[1]), 4)
    _check_device_floats("Denoise: rgba", rgba, shape)
    _check_device_floats("Denoise: aov", aov, shape)
    out = _aov_out("Denoise", out, shape)
    p = make_c_denoise_params(params)
    L = load_library()
    n = L.nrc_denoise_scratch_bytes(C.c_uint32(shape[1]), C.c_uint32(shape[0]), C.byref(p))
    if n == 0:
        raise RuntimeError(L.nrc_last_error().decode() or "denoise: refused")
    scratch = torch.empty(n, device="cuda", dtype=torch.uint8)
    stream = torch.cuda.current_stream()
    _check(L.nrc_denoise(_dev_ptr(rgba), _dev_ptr(aov), C.c_uint32(shape[1]), C.c_uint32(shape[0]), C.byref(p), _dev_ptr(out), _dev_ptr(scratch),
                         C.c_void_p(stream.cuda_stream)))
    scratch.record_stream(stream)
    return out


def test_denoise_host(rgba, aov, params=None):
    """nrc_test_denoise_host: the filter [h][w][4] (numpy) of the numpy images rgba and aov [h][w][4], computed on the CPU inside the library
    by csrc/nrc_denoise.hpp's arithmetic"""
    c = np.ascontiguousarray(rgba, np.float32)
    g = np.ascontiguousarray(aov, np.float32)
    if c.ndim != 3 or c.shape[2] != 4 or g.shape != c.shape:
        raise ValueError("test_denoise_host: rgba and aov must both be [h][w][4]")
    out = np.empty_like(c)
    p = make_c_denoise_params(params)
    _check(load_library().nrc_test_denoise_host(c.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), C.c_uint32(c.shape[1]),
                                                C.c_uint32(c.shape[0]), C.byref(p), out.ctypes.data_as(C.c_void_p)))
    return out


class NrcReprojectParams(C.Structure):
    _fields_ = [("max_history", C.c_float), ("sigma_alpha", C.c_float), ("sigma_depth", C.c_float)]


def make_c_reproject_params(params=None):
    """nrc_reproject_params: the library's defaults (nrc_reproject_params_default) overridden by `params` -- None, a dict with any of
    max_history, sigma_alpha, sigma_depth (scene.reproject_params), or an NrcReprojectParams.  The library checks the values."""
    if isinstance(params, NrcReprojectParams):
        return params
    p = NrcReprojectParams()
    load_library().nrc_reproject_params_default(C.byref(p))
    for k, v in (params or {}).items():
        if k not in ("max_history", "sigma_alpha", "sigma_depth"):
            raise ValueError("reproject parameters: unknown key %r" % (k,))
        setattr(p, k, float(v))
    return p


def _reproject_history(what, hist):
    """`hist` of Reproject / test_reproject_host: None, or the four of (rgba, count, aov, camera)"""
    if hist is None:
        return None
    if not isinstance(hist, (tuple, list)) or len(hist) != 4:
        raise ValueError("%s: hist must be None or (rgba, count, aov, camera)" % what)
    return tuple(hist)


def Reproject(hist, rgba, frames, aov, camera, params=None, out=None, out_count=None):
    """nrc_reproject: history reuse by reprojection (include/nrc_hpm.h, "Reproject") over whole images.  hist: None (no history: the result
    is rgba and frames) or (rgba, count, aov, camera) of the history view -- contiguous float32 CUDA tensors [h][w][4], [h][w], [h][w][4]
    and a camera (scene.make_camera); rgba, aov: the current view's frame and view AOV, `frames` the number of frames blended into rgba,
    camera its camera; params as for make_c_reproject_params.  Returns (out [h][w][4], count [h][w]) -- `out` / `out_count`, or new tensors;
    never an input.  Opt-in and biased.  Enqueued on torch's current stream; no host wait."""
    import torch
    if not isinstance(rgba, torch.Tensor) or rgba.dim() != 3:
        raise ValueError("Reproject: rgba must be a contiguous float32 CUDA tensor of shape (h, w, 4)")
    shape = (int(rgba.shape[0]), int(rgba.shape[1]), 4)
    _check_device_floats("Reproject: rgba", rgba, shape)
    _check_device_floats("Reproject: aov", aov, shape)
    hist = _reproject_history("Reproject", hist)
    hp = [None, None, None, None]
    if hist is not None:
        _check_device_floats("Reproject: hist rgba", hist[0], shape)
        _check_device_floats("Reproject: hist count", hist[1], shape[:2])
        _check_device_floats("Reproject: hist aov", hist[2], shape)
        hcam = make_c_camera(hist[3])
        hp = [_dev_ptr(hist[0]), _dev_ptr(hist[1]), _dev_ptr(hist[2]), C.byref(hcam)]
    out = _aov_out("Reproject", out, shape)
    out_count = _aov_out("Reproject: count", out_count, shape[:2])
    p = make_c_reproject_params(params)
    cam = make_c_camera(camera)
    _check(load_library().nrc_reproject(hp[0], hp[1], hp[2], hp[3], _dev_ptr(rgba), C.c_float(frames), _dev_ptr(aov), C.byref(cam), C.c_uint32(shape[1]),
                                        C.c_uint32(shape[0]), C.byref(p), _dev_ptr(out), _dev_ptr(out_count),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out, out_count


def test_reproject_host(hist, rgba, frames, aov, camera, params=None):
    """nrc_test_reproject_host: (out [h][w][4], count [h][w]) (numpy) of Reproject's arguments as numpy arrays, computed on the CPU inside the
    library by csrc/nrc_reproject.hpp's arithmetic"""
    c = np.ascontiguousarray(rgba, np.float32)
    g = np.ascontiguousarray(aov, np.float32)
    if c.ndim != 3 or c.shape[2] != 4 or g.shape != c.shape:
        raise ValueError("test_reproject_host: rgba and aov must both be [h][w][4]")
    hist = _reproject_history("test_reproject_host", hist)
    hp = [None, None, None, None]
    if hist is not None:
        hc, hn, hg = np.ascontiguousarray(hist[0], np.float32), np.ascontiguousarray(hist[1], np.float32), np.ascontiguousarray(hist[2], np.float32)
        if hc.shape != c.shape or hg.shape != c.shape or hn.shape != c.shape[:2]:
            raise ValueError("test_reproject_host: the history must be [h][w][4], [h][w], [h][w][4]")
        hcam = make_c_camera(hist[3])
        hp = [hc.ctypes.data_as(C.c_void_p), hn.ctypes.data_as(C.c_void_p), hg.ctypes.data_as(C.c_void_p), C.byref(hcam)]
    out, count = np.empty_like(c), np.empty(c.shape[:2], np.float32)
    p = make_c_reproject_params(params)
    cam = make_c_camera(camera)
    _check(load_library().nrc_test_reproject_host(hp[0], hp[1], hp[2], hp[3], c.ctypes.data_as(C.c_void_p), C.c_float(frames), g.ctypes.data_as(C.c_void_p),
                                                  C.byref(cam), C.c_uint32(c.shape[1]), C.c_uint32(c.shape[0]), C.byref(p),
                                                  out.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p)))
    return out, count


class NrcOrthoView(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("dir", C.c_float * 3)]


def make_c_ortho_view(view):
    """nrc_ortho_view of a dict {origin, du, dv, dir} (scene.light_view)"""
    v = NrcOrthoView()
    for k in ("origin", "du", "dv", "dir"):
        a = np.asarray(view[k], np.float32).reshape(-1)
        if a.size != 3:
            raise ValueError("ortho view: %s must hold 3 numbers" % k)
        getattr(v, k)[:] = [float(x) for x in a]
    return v


def _times_keyword(plain):
    """RenderPath(..., times=None, aov_out=None, aov_depths=None, denoised_out=None, denoise_params=None, accumulated_out=None,
    accumulated_counts=None, reproject_params=None) of both renderers.  The keywords ride on the untimed method: its positional signature is
    a published one (callers and tests/test_camera_path_host.py name its parameters in order) and stays what inspect.signature reports; a
    call without times is `plain`'s own, a call with times goes to the renderer's _path with the same arguments.
    aov_out: a contiguous float32 CUDA tensor [len(cameras)][height][width][4] that receives every view's AOV ({alpha, tau, z_front,
    z_half} of that view's camera and medium: ViewAov, nrc_renderer_set_path_aov_target); frames, `out` and training are unchanged by it.
    aov_depths (with aov_out): a contiguous float32 CUDA tensor [len(cameras)][height][width]; view i's AOV is held out to aov_depths[i]
    (ViewAovToDepth, nrc_renderer_set_path_aov_depths).
    denoised_out (with aov_out, without aov_depths): a tensor of aov_out's shape that receives every view's final frame filtered with the
    view's own AOV (DenoisedFrame, nrc_renderer_set_path_denoise_target); denoise_params as for make_c_denoise_params.
    accumulated_out (with aov_out, without aov_depths): a tensor of aov_out's shape that receives every view's frame accumulated over the
    views before it by reprojection (Reproject, nrc_renderer_set_path_reproject_target); accumulated_counts: a tensor
    [len(cameras)][height][width] for the effective frame counts (None: one is made and dropped); reproject_params as for
    make_c_reproject_params.  With denoised_out too, the filter reads the accumulated frames."""
    @functools.wraps(plain)
    def RenderPath(self, *args, times=None, aov_out=None, aov_depths=None, denoised_out=None, denoise_params=None, accumulated_out=None,
                   accumulated_counts=None, reproject_params=None, **kw):
        bound = inspect.signature(plain).bind(self, *args, **kw)
        bound.apply_defaults()
        if accumulated_counts is not None and accumulated_out is None:      # (before any target is set)
            raise ValueError("RenderPath: accumulated_counts needs accumulated_out")
        if aov_out is not None:
            import torch
            shape = (len(list(bound.arguments["cameras"])), self.height, self.width, 4)
            if not isinstance(aov_out, torch.Tensor) or not aov_out.is_cuda or aov_out.dtype != torch.float32 \
                    or tuple(aov_out.shape) != shape or not aov_out.is_contiguous():
                raise ValueError("RenderPath: aov_out must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
            self.SetPathAovTarget(aov_out)
        if aov_depths is not None:
            if aov_out is None:
                raise ValueError("RenderPath: aov_depths needs aov_out")
            try:
                _check_device_floats("RenderPath: aov_depths", aov_depths, shape[:3])
            except ValueError:
                self.SetPathAovTarget(None)
                raise
            self.SetPathAovDepths(aov_depths)
        if denoised_out is not None:
            try:
                if aov_out is None:
                    raise ValueError("RenderPath: denoised_out needs aov_out (a view's AOV is its guide)")
                _check_device_floats("RenderPath: denoised_out", denoised_out, shape)
                self.SetPathDenoiseTarget(denoised_out, denoise_params)
            except Exception:
                if aov_out is not None:
                    self.SetPathAovTarget(None)
                if aov_depths is not None:
                    self.SetPathAovDepths(None)
                raise
        if accumulated_out is not None:
            try:
                if aov_out is None:
                    raise ValueError("RenderPath: accumulated_out needs aov_out (the views' AOVs are the guides)")
                _check_device_floats("RenderPath: accumulated_out", accumulated_out, shape)
                if accumulated_counts is None:
                    import torch
                    accumulated_counts = torch.empty(shape[:3], device="cuda", dtype=torch.float32)
                _check_device_floats("RenderPath: accumulated_counts", accumulated_counts, shape[:3])
                self.SetPathReprojectTarget(accumulated_out, accumulated_counts, reproject_params)
            except Exception:
                if aov_out is not None:
                    self.SetPathAovTarget(None)
                if aov_depths is not None:
                    self.SetPathAovDepths(None)
                if denoised_out is not None:
                    self.SetPathDenoiseTarget(None)
                raise
        try:
            if times is None:
                return plain(self, *args, **kw)
            return self._path(*list(bound.arguments.values())[1:], times)
        finally:
            if aov_out is not None:      # (consumed by the path call; a call that failed before it reached the library leaves none behind)
                self.SetPathAovTarget(None)
            if aov_depths is not None:
                self.SetPathAovDepths(None)
            if denoised_out is not None:
                self.SetPathDenoiseTarget(None)
            if accumulated_out is not None:
                self.SetPathReprojectTarget(None, None)
    return RenderPath


class _LiveMedium:
    """The medium of a live renderer: what NrcHpmRenderer and McHpmRenderer share (include/nrc_hpm.h declares every call once per renderer,
    nrc_renderer_* and nrc_mc_renderer_*: _PREFIX is the class's).  Uses the renderer's self.L, self.h and self._scene."""
    _PREFIX = None

    def _medium(self, name):
        return getattr(self.L, self._PREFIX + name)

    def TileMask(self):
        """the empty-space tile mask in use (numpy uint32: the bit words + the trailing "off for this camera" word; empty: no mask in use);
        synchronises the renderer"""
        fn = self._medium("tile_mask")
        n = fn(self.h, None, C.c_size_t(0))
        out = np.zeros(n, np.uint32)
        if n and fn(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)) != n:
            raise RuntimeError(self.L.nrc_last_error().decode() or "tile_mask failed")
        return out

    def TileFar(self):
        """the far bounds built with that mask (numpy float32, one per 8x8 tile, row-major; empty: no mask in use): see
        nrc_renderer_tile_far; synchronises the renderer"""
        fn = self._medium("tile_far")
        n = fn(self.h, None, C.c_size_t(0))
        out = np.zeros(n, np.float32)
        if n and fn(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n)) != n:
            raise RuntimeError(self.L.nrc_last_error().decode() or "tile_far failed")
        return out

    def ViewAov(self):
        """the view AOV of the current camera and medium (include/nrc_hpm.h, "View AOV"): a torch CUDA tensor view [height, width, 4] of
        {alpha, tau, z_front, z_half} per pixel -- exact opacity 1 - exp(-tau), optical depth, distance to the first non-empty voxel and
        to optical depth ln 2 along the pixel's camera ray (+inf where undefined).  Computed at most once per change of camera, volume
        or scene parameters, on the renderer's stream; the stream given at construction is ordered behind it.  The tensor is the
        renderer's buffer: the next ViewAov() after a change rewrites it."""
        import torch
        p = self._medium("view_aov")(self.h)
        if not p:
            raise RuntimeError(self.L.nrc_last_error().decode() or "view_aov failed")
        return _wrap_device(p, self.width * self.height * 16, torch.float32, (self.height, self.width, 4))

    def SetPathAovTarget(self, aovs, views=None):
        """nrc_renderer_set_path_aov_target: the next RenderPath writes view i's AOV to aovs[i] (a contiguous float32 CUDA tensor
        [views][height][width][4]; None cancels).  RenderPath(..., aov_out=) makes this call itself."""
        if aovs is None:
            _check(self._medium("set_path_aov_target")(self.h, None, C.c_uint32(0)))
        else:
            _check(self._medium("set_path_aov_target")(self.h, _dev_ptr(aovs), C.c_uint32(int(aovs.shape[0]) if views is None else int(views))))

    def SetPathAovDepths(self, depths, views=None):
        """nrc_renderer_set_path_aov_depths: with an AOV target set, the next RenderPath holds view i's AOV out to depths[i] (a contiguous
        float32 CUDA tensor [views][height][width]; None cancels).  RenderPath(..., aov_out=, aov_depths=) makes this call itself."""
        if depths is None:
            _check(self._medium("set_path_aov_depths")(self.h, None, C.c_uint32(0)))
        else:
            _check(self._medium("set_path_aov_depths")(self.h, _dev_ptr(depths), C.c_uint32(int(depths.shape[0]) if views is None else int(views))))

    def _aov(self, what, source, arg, levels=None, out=None, flat=None):
        """What the ray AOV's and the deep AOV's methods share.  source / arg: "rays" / the [n][8] tensor, "depth" / the view's depth image
        (None: whole rays, the deep call only) or "ortho" / (view, w, h); it sets the rays' shape and the head of the C call.
        levels None: the flat call, the result [*shape][4] in `out` or a new tensor.  Otherwise the deep call nrc_*_deep_*: the planes
        [K][*shape] in `out` or a new tensor, and (planes, flat) when a flat result is asked for."""
        import torch
        deep = levels is not None
        if source == "rays":
            if not isinstance(arg, torch.Tensor) or arg.dim() != 2:
                raise ValueError("%s: rays must be a contiguous float32 CUDA tensor of shape (n, 8)" % what)
            _check_device_floats(what + ": rays", arg, (arg.shape[0], 8))
            shape = (int(arg.shape[0]),)
            name, head = "ray_aov", (C.c_size_t(shape[0]), _dev_ptr(arg))
        elif source == "depth":
            shape = (self.height, self.width)
            if arg is not None or not deep:
                _check_device_floats(what + ": depth", arg, shape)
            name, head = ("view_aov" if deep else "view_aov_to_depth"), (_dev_ptr(arg) if arg is not None else None,)
        else:
            view, w, h = arg[0], int(arg[1]), int(arg[2])
            if w <= 0 or h <= 0:
                raise ValueError("%s: the image size must be positive" % what)
            v = make_c_ortho_view(view)
            shape = (h, w)
            name, head = "ortho_aov", (C.byref(v), C.c_uint32(w), C.c_uint32(h))
        if not deep:
            out = _aov_out(what, out, shape + (4,))
            _check(self._medium(name)(self.h, *head, _dev_ptr(out)))
            return out
        lv, k = _deep_levels_arg(levels)
        out = _aov_out(what, out, (k,) + shape)
        flat = _deep_flat(what, flat, shape + (4,))
        if shape[0] != 0:      # (no rays, no work -- and an empty tensor has no address for the library's NULL check)
            _check(self._medium("deep_" + name)(self.h, *head, C.c_uint32(k), lv.ctypes.data_as(C.c_void_p), _dev_ptr(out),
                                                _dev_ptr(flat) if flat is not None else None))
        return out if flat is None else (out, flat)

    def RayAov(self, rays, out=None):
        """the ray AOV of a list of segments through the current medium (include/nrc_hpm.h, "Ray AOV"; nrc_renderer_ray_aov): rays is a
        contiguous float32 CUDA tensor [n][8] of {ox, oy, oz, t_min, dx, dy, dz, t_max}, the result [n][4] of {alpha, tau, z_front, z_half}
        (`out`, or a new tensor).  One launch on the renderer's stream, no host wait."""
        return self._aov("RayAov", "rays", rays, out=out)

    def ViewAovToDepth(self, depth, out=None):
        """the view AOV held out to a depth image (nrc_renderer_view_aov_to_depth): depth is a contiguous float32 CUDA tensor
        [height][width], the distance along each pixel's camera ray (the unit of z_front) at which the ray ends; +inf gives ViewAov()'s
        bits, a depth <= 0 or NaN the empty result.  Returns [height][width][4] (`out`, or a new tensor)."""
        return self._aov("ViewAovToDepth", "depth", depth, out=out)

    def OrthoAov(self, view, w, h, out=None):
        """the ray AOV of an orthographic view {origin, du, dv, dir} (scene.light_view: the medium's shadow map) of w x h pixels, whatever
        the renderer's size (nrc_renderer_ortho_aov).  Returns [h][w][4] (`out`, or a new tensor)."""
        return self._aov("OrthoAov", "ortho", (view, w, h), out=out)

    def DeepRayAov(self, rays, levels, out=None, flat=None):
        """the deep AOV of a list of segments (include/nrc_hpm.h, "Deep AOV"; nrc_renderer_deep_ray_aov): rays as for RayAov, levels the
        K optical depths (scene.deep_levels; ascending, positive, K <= 32).  Returns the planes [K][n] -- z[k][i]: the ray parameter at which
        ray i reaches levels[k], +inf where it never does -- in `out` or a new tensor.  flat: None, True (a new tensor) or a tensor [n][4]
        that receives RayAov's result of the same walk; with it the return value is (planes, flat).  One launch, no host wait."""
        return self._aov("DeepRayAov", "rays", rays, levels, out, flat)

    def DeepViewAov(self, levels, depth=None, out=None, flat=None):
        """the deep AOV of every pixel's camera ray (nrc_renderer_deep_view_aov): a deep image's samples, planes [K][height][width].
        depth: None (whole rays) or a depth image as for ViewAovToDepth.  flat as for DeepRayAov, [height][width][4]."""
        return self._aov("DeepViewAov", "depth", depth, levels, out, flat)

    def DeepOrthoAov(self, view, w, h, levels, out=None, flat=None):
        """the deep AOV of an orthographic view (scene.light_view): a deep shadow map, planes [K][h][w] (nrc_renderer_deep_ortho_aov).
        flat as for DeepRayAov, [h][w][4]."""
        return self._aov("DeepOrthoAov", "ortho", (view, w, h), levels, out, flat)

    def DenoisedFrame(self, params=None):
        """the current framebuffer filtered with the current view AOV (include/nrc_hpm.h, "Denoise"; nrc_renderer_denoised_frame): a torch
        CUDA tensor view [height, width, 4].  Opt-in and biased: for low frame counts and previews.  Enqueued behind the frames rendered
        so far, no host wait; the stream given at construction is ordered behind it.  The tensor is the renderer's buffer: the next
        DenoisedFrame() rewrites it.  A renderer that draws a strip of a sharded frame refuses."""
        import torch
        p = make_c_denoise_params(params)
        ptr = self._medium("denoised_frame")(self.h, C.byref(p))
        if not ptr:
            raise RuntimeError(self.L.nrc_last_error().decode() or "denoised_frame failed")
        return _wrap_device(ptr, self.width * self.height * 16, torch.float32, (self.height, self.width, 4))

    def SetPathDenoiseTarget(self, denoised, params=None, views=None):
        """nrc_renderer_set_path_denoise_target: the next RenderPath writes view i's filtered final frame to denoised[i] (a contiguous
        float32 CUDA tensor [views][height][width][4]; None cancels).  Needs an AOV target in the same call and no AOV depths.
        RenderPath(..., aov_out=, denoised_out=) makes this call itself."""
        if denoised is None:
            _check(self._medium("set_path_denoise_target")(self.h, None, C.c_uint32(0), None))
        else:
            p = make_c_denoise_params(params)
            _check(self._medium("set_path_denoise_target")(self.h, _dev_ptr(denoised), C.c_uint32(int(denoised.shape[0]) if views is None else int(views)),
                                                           C.byref(p)))

    def SetPathReprojectTarget(self, accum, counts, params=None, views=None):
        """nrc_renderer_set_path_reproject_target: the next RenderPath writes view i's frame, accumulated over the views before it by
        reprojection, to accum[i] and its effective frame counts to counts[i] (contiguous float32 CUDA tensors [views][height][width][4]
        and [views][height][width]; accum None cancels).  Needs an AOV target in the same call and no AOV depths.
        RenderPath(..., aov_out=, accumulated_out=) makes this call itself."""
        if accum is None:
            _check(self._medium("set_path_reproject_target")(self.h, None, None, C.c_uint32(0), None))
        else:
            p = make_c_reproject_params(params)
            _check(self._medium("set_path_reproject_target")(self.h, _dev_ptr(accum), _dev_ptr(counts) if counts is not None else None,
                                                             C.c_uint32(int(accum.shape[0]) if views is None else int(views)), C.byref(p)))

    def ExportDenoisedImageToFile(self, filePath, params=None):
        """ExportImageWithAovToFile with B, G, R taken from DenoisedFrame(params) (nrc_renderer_export_exr_denoised)"""
        p = make_c_denoise_params(params)
        _check(self._medium("export_exr_denoised")(self.h, filePath.encode(), C.byref(p)))

    def ExportImageWithAovToFile(self, filePath):
        """ExportOutputImageToFile with the view AOV beside the colours: a scan-line EXR with FLOAT channels A (alpha of the AOV), B, G, R,
        Z (z_front), Zhalf, tau (io_exr.read_exr_channels; io_exr.read_exr still finds RGBA).  This renderer's pixels only."""
        _check(self._medium("export_exr_aov")(self.h, filePath.encode()))

    def SetSceneParams(self, scene):
        """lights / medium constants of `scene` (dict of scene.make_scene or scene.HpmScene); textures are not re-uploaded"""
        sc_ = make_c_scene(scene.scene if hasattr(scene, "scene") else scene)
        _check(self._medium("set_scene_params")(self.h, C.byref(sc_)))

    def SetVolume(self, vol):
        """a new density volume with the creation dims (include/nrc_hpm.h, nrc_renderer_set_volume): frames rendered from now on see it,
        blending restarts, the cache keeps its weights.  vol: a C-contiguous numpy uint8 [nz][ny][nx] array (host memory: the call copies
        it and waits for the copy) or a contiguous CUDA torch tensor, uint8 or float32 [nz][ny][nx] (read on the renderer's stream; the call
        does not wait)"""
        fn = self._medium("set_volume")
        if isinstance(vol, np.ndarray):
            if vol.dtype != np.uint8 or vol.ndim != 3 or not vol.flags.c_contiguous:
                raise RuntimeError("SkyRenderer ERROR: SetVolume takes a C-contiguous uint8 numpy array [nz][ny][nx] (got %s %s)" % (vol.dtype, vol.shape))
            nz, ny, nx = vol.shape
            _check(fn(self.h, C.c_void_p(vol.ctypes.data), nx, ny, nz, VOLUME_U8, 0))
            return
        import torch
        if not isinstance(vol, torch.Tensor) or not vol.is_cuda or vol.dim() != 3 or not vol.is_contiguous() \
                or vol.dtype not in (torch.uint8, torch.float32):
            raise RuntimeError("SkyRenderer ERROR: SetVolume takes a contiguous CUDA tensor, uint8 or float32 [nz][ny][nx], or a uint8 numpy array")
        nz, ny, nx = vol.shape
        _check(fn(self.h, _dev_ptr(vol), nx, ny, nz, VOLUME_F32 if vol.dtype == torch.float32 else VOLUME_U8, 1))

    def SetVolumeBricks(self, origins, bricks):
        """the same from 8^3 bricks (include/nrc_hpm.h, nrc_renderer_set_volume_bricks; scene.volume_to_bricks makes them of a dense volume):
        origins int32 [n][3] (x, y, z: multiples of 8), bricks uint8 or float32 [n][8][8][8], two numpy arrays or two CUDA tensors (_brick_list);
        voxels no brick covers become 0, n = 0 is the empty medium"""
        _check(self._medium("set_volume_bricks")(self.h, *_brick_list("SetVolumeBricks", origins, bricks)))

    def SetVolumeKeys(self, keys):
        """volume keyframes (include/nrc_hpm.h, nrc_renderer_set_volume_keys): keys [n_keys][nz][ny][nx] of the creation dims, uint8 or
        float32, a C-contiguous numpy array (host memory: the call copies it and waits for the copy) or a contiguous CUDA torch tensor
        (read on the renderer's stream; the call does not wait for that); key i sits at time i.  The renderer keeps its own R8 copy on the
        device.  None or an array of no keys drops the sequence.  Not a per-frame call: it may wait for the frames in flight."""
        fn = self._medium("set_volume_keys")
        if keys is None:
            _check(fn(self.h, None, 0, 0, 0, 0, VOLUME_U8, 0))
            return
        if isinstance(keys, np.ndarray):
            if keys.dtype not in (np.uint8, np.float32) or keys.ndim != 4 or not keys.flags.c_contiguous:
                raise RuntimeError("SkyRenderer ERROR: SetVolumeKeys takes a C-contiguous uint8 or float32 numpy array [n_keys][nz][ny][nx] (got %s %s)"
                                   % (keys.dtype, keys.shape))
            n, nz, ny, nx = keys.shape
            _check(fn(self.h, C.c_void_p(keys.ctypes.data) if n else None, n, nx, ny, nz, VOLUME_F32 if keys.dtype == np.float32 else VOLUME_U8, 0))
            return
        import torch
        if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dim() != 4 or not keys.is_contiguous() \
                or keys.dtype not in (torch.uint8, torch.float32):
            raise RuntimeError("SkyRenderer ERROR: SetVolumeKeys takes a contiguous CUDA tensor or a numpy array, uint8 or float32 [n_keys][nz][ny][nx]")
        n, nz, ny, nx = keys.shape
        _check(fn(self.h, _dev_ptr(keys) if n else None, n, nx, ny, nz, VOLUME_F32 if keys.dtype == torch.float32 else VOLUME_U8, 1))

    def SetVolumeKeyBricks(self, counts, origins, bricks):
        """the same sequence held as 8^3 brick lists (include/nrc_hpm.h, nrc_renderer_set_volume_key_bricks; scene.volumes_to_key_bricks makes
        the three of dense keys): counts = bricks per key, origins int32 [sum][3] and bricks uint8 or float32 [sum][8][8][8] the keys' lists
        in key order, numpy arrays or CUDA tensors.  It replaces a dense sequence and the other way round; counts None drops the sequence.
        Not a per-frame call."""
        _set_volume_key_bricks(self._medium("set_volume_key_bricks"), self.h, counts, origins, bricks)

    def VolumeKeyBytes(self):
        """the device bytes the current key sequence holds (dense: n_keys * nx*ny*nz; bricks: 512 * sum(counts) + 4 * n_keys * cells)"""
        return int(self._medium("volume_key_bytes")(self.h))

    def VolumeKeyCount(self):
        return int(self._medium("volume_key_count")(self.h))

    def SetVolumeTime(self, t):
        """the medium becomes the in-between of the two keys around time t, 0 <= t <= VolumeKeyCount() - 1 (scene.volume_at is the CPU
        statement): what SetVolume of that volume does, without a host wait"""
        _check(self._medium("set_volume_time")(self.h, C.c_float(float(t))))

    def VolumeBuffer(self, name):
        """device view of the current volume's buffers (after synchronising the renderer): 'density' uint8 [nz][ny][nx], 'occ_bits' int32
        words, 'boxes' float32 [n][6]"""
        import torch
        if name not in VOLUME_BUF:
            raise RuntimeError("SkyRenderer ERROR: VolumeBuffer name must be one of %s" % sorted(VOLUME_BUF))
        nbytes = C.c_size_t(0)
        p = self._medium("volume_buffer")(self.h, C.c_int(VOLUME_BUF[name]), C.byref(nbytes))
        if not p:
            if name == "boxes" and not self.L.nrc_last_error():
                return torch.zeros((0, 6), dtype=torch.float32, device="cuda")
            _check(-1)
        if name == "density":
            return _wrap_device(p, nbytes.value, torch.uint8, (self._scene.nz, self._scene.ny, self._scene.nx))
        if name == "occ_bits":
            return _wrap_device(p, nbytes.value, torch.int32, (nbytes.value // 4,))
        return _wrap_device(p, nbytes.value, torch.float32, (nbytes.value // 24, 6))


# ------------------------------------------------------------------------------------------------------------------
class NeuralRadianceCache:
    """en::NeuralRadianceCache (src/NeuralRadianceCache.cu)."""
    MASTER, EMA, ADAM_M, ADAM_V, GRAD = range(5)

    def __init__(self, appConfig):
        self.L = load_library()
        self.cfg = appConfig
        h = C.c_void_p()
        _check(self.L.nrc_cache_create(C.byref(appConfig.c), C.byref(h)))
        self.h = h
        self._hook_keep = None
        self._bufs = None

    def Init(self, inferCount, dInferInput, dInferOutput, dTrainInput, dTrainTarget, stream=None, cudaStartEvent=None,
             cudaFinishedEvent=None):
        """Buffers: torch CUDA float32 tensors [n,5] / [n,3] (caller-owned, as in the reference).  cudaStartEvent /
        cudaFinishedEvent: torch.cuda.Event objects standing in for the reference's two external semaphores
        (include/engine/graphics/NeuralRadianceCache.hpp:15-22): InferAndTrain waits for the first and records the second."""
        self._bufs = (dInferInput, dInferOutput, dTrainInput, dTrainTarget, cudaStartEvent, cudaFinishedEvent)
        if cudaStartEvent is None and cudaFinishedEvent is None:
            _check(self.L.nrc_cache_init(self.h, C.c_uint32(inferCount), _dev_ptr(dInferInput), _dev_ptr(dInferOutput),
                                         _dev_ptr(dTrainInput), _dev_ptr(dTrainTarget), _stream_ptr(stream)))
            return
        ev = [C.c_void_p(int(e.cuda_event)) if e is not None else None for e in (cudaStartEvent, cudaFinishedEvent)]
        _check(self.L.nrc_cache_init_events(self.h, C.c_uint32(inferCount), _dev_ptr(dInferInput), _dev_ptr(dInferOutput),
                                            _dev_ptr(dTrainInput), _dev_ptr(dTrainTarget), _stream_ptr(stream), ev[0], ev[1]))

    def InferAndTrain(self, inferFilter, train):
        f = None
        if inferFilter is not None:
            f = np.ascontiguousarray(inferFilter, np.uint32)
        _check(self.L.nrc_cache_infer_and_train(self.h, f.ctypes.data_as(C.c_void_p) if f is not None else None,
                                                C.c_int(int(bool(train)))))

    def Destroy(self):
        if self.h:
            _check(self.L.nrc_cache_destroy(self.h))
            self.h = None

    def GetLoss(self, wait=True):
        """en::NeuralRadianceCache::GetLoss(): the loss of the last training step enqueued (src/NeuralRadianceCache.cu:154; waits for
        that step only).  wait=False = GetLossAsync()[0]."""
        if wait:
            return float(self.L.nrc_cache_get_loss(self.h))
        return self.GetLossAsync()[0]

    def GetLossAsync(self):
        """never blocks: (loss of the most recent COMPLETED step, that step's number, number of the newest step enqueued) -- the
        per-frame poll of src/main.cu:303,376 without draining the frame pipeline"""
        loss, step, enq = C.c_float(0), C.c_uint32(0), C.c_uint32(0)
        _check(self.L.nrc_cache_get_loss_async(self.h, C.byref(loss), C.byref(step), C.byref(enq)))
        return float(loss.value), int(step.value), int(enq.value)

    def GetInferBatchCount(self):
        return int(self.L.nrc_cache_get_infer_batch_count(self.h))

    def GetTrainBatchCount(self):
        return int(self.L.nrc_cache_get_train_batch_count(self.h))

    def GetInferBatchSize(self):
        return int(self.L.nrc_cache_get_infer_batch_size(self.h))

    def GetTrainBatchSize(self):
        return int(self.L.nrc_cache_get_train_batch_size(self.h))

    # ---- finer-grained steps (multi-GPU driver, tests) ----
    def SetStream(self, stream=None):
        _check(self.L.nrc_cache_set_stream(self.h, _stream_ptr(stream)))

    def Infer(self, dInput, dOutput, useEma=True):
        _check(self.L.nrc_cache_infer(self.h, _dev_ptr(dInput), _dev_ptr(dOutput), C.c_uint32(dInput.shape[0]),
                                      C.c_int(int(useEma))))

    def Backward(self, dInput, dTarget, nNorm=0):
        _check(self.L.nrc_cache_backward(self.h, _dev_ptr(dInput), _dev_ptr(dTarget), C.c_uint32(dInput.shape[0]),
                                         C.c_uint32(nNorm)))

    def OptimizerStep(self):
        _check(self.L.nrc_cache_optimizer_step(self.h))

    def ParamCount(self):
        return int(self.L.nrc_cache_param_count(self.h))

    def GradTensor(self):
        import torch
        n = self.ParamCount()
        return _wrap_device(self.L.nrc_cache_grad_ptr(self.h), n * 4, torch.float32, (n,))

    def LossTensor(self):
        import torch
        return _wrap_device(self.L.nrc_cache_loss_ptr(self.h), 8, torch.float32, (2,))

    def CommInit(self, unique_id, rank, world):
        """native RCCL gradient exchange: unique_id = 128 bytes from comm_unique_id() of rank 0 (collective call)"""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        _check(self.L.nrc_cache_comm_init(self.h, buf, C.c_int(rank), C.c_int(world)))

    def CommInfo(self):
        """(rank, world) as the library's RCCL communicator reports them; world 0 = no native communicator"""
        r, w = C.c_int(0), C.c_int(0)
        _check(self.L.nrc_cache_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def CommTimeExchange(self, reps=100):
        """average microseconds of one gradient all-reduce of the native exchange (collective call; 0.0 without a communicator)"""
        us = C.c_float(0)
        _check(self.L.nrc_cache_comm_time_exchange(self.h, C.c_uint32(reps), C.byref(us)))
        return float(us.value)

    def CommSparse(self):
        """True when the HashGrid table gradient travels as (entry, value) lists (native exchange of a posID 0 model)"""
        return bool(self.L.nrc_cache_comm_sparse(self.h))

    def GridGradPack(self):
        """(debug) the table gradient of the last Backward as the exchange list: uint32 words {count, 0, (entry, half2 bits) x
        capacity}, padding entries 0xffffffff"""
        cap = int(self.L.nrc_cache_grid_list_capacity(self.h))
        out = np.zeros(2 + 2 * cap, np.uint32)
        _check(self.L.nrc_cache_grid_grad_pack(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size)))
        return out

    def GridGradApply(self, lists):
        """(debug) gradient vector's table part := sum of the lists (GridGradPack layout), added in the order given"""
        v = np.ascontiguousarray(np.stack(lists), np.uint32)
        _check(self.L.nrc_cache_grid_grad_apply(self.h, v.ctypes.data_as(C.c_void_p), C.c_uint32(v.shape[0])))

    def SetExchangeDtype(self, dtype):
        """nrc_cache_set_exchange_dtype: "f32" (default) or "f16" -- the gradients summed over the ranks as fp16 numbers pre-scaled by
        loss_scale 128 (BASELINE.json configs[3]); every rank alike"""
        _check(self.L.nrc_cache_set_exchange_dtype(self.h, C.c_int({"f32": 0, "f16": 1}[dtype])))

    def GetExchangeDtype(self):
        return "f16" if self.L.nrc_cache_get_exchange_dtype(self.h) == 1 else "f32"

    def SetNonFinitePolicy(self, policy):
        """nrc_cache_set_nonfinite_policy: NRC_NONFINITE_PROPAGATE (default) or NRC_NONFINITE_SKIP -- a training step whose loss or
        gradient is not finite leaves weights, EMA weights and Adam moments as they are and is counted; every rank alike"""
        _check(self.L.nrc_cache_set_nonfinite_policy(self.h, C.c_int(int(policy))))

    def GetNonFinitePolicy(self):
        return int(self.L.nrc_cache_get_nonfinite_policy(self.h))

    def GetSkippedSteps(self):
        """(number of steps skipped so far, step number of the last one skipped; 0 = none) -- waits for the last enqueued step only"""
        n, last = C.c_uint32(0), C.c_uint32(0)
        _check(self.L.nrc_cache_get_skipped_steps(self.h, C.byref(n), C.byref(last)))
        return int(n.value), int(last.value)

    def SetLossNormFactor(self, factor):
        _check(self.L.nrc_cache_set_loss_norm_factor(self.h, C.c_uint32(factor)))

    def SetGradHook(self, fn):
        """fn(grad_tensor, loss_tensor) is called between backward and the optimizer of every train batch, with torch's
        current stream switched to the stream the training kernels are ordered on."""
        if fn is None:
            self._hook_keep = None
            _check(self.L.nrc_cache_set_grad_hook(self.h, None, None))
            return
        g, lo = self.GradTensor(), self.LossTensor()

        import torch

        def tramp(_user, _g, _n, _l, stream):
            s = torch.cuda.ExternalStream(int(stream or 0))
            with torch.cuda.stream(s):
                fn(g, lo)
                # What fn enqueued through torch must be COMPLETE when the library launches its next kernel on the stream.  Measured (round 6,
                # tools/_build/bisect_flaky.sh): an in-place torch kernel launched here on this very stream overlapped the library's next
                # kernel on it -- 300..4 700 of 25 792 gradient words kept their old value -- whenever tests/test_gpu_frame_graph.py had run
                # in the same process before (3 of 3), never in a fresh process whatever the number of streams or hardware queues
                # (tools/_build/hook_overlap_probe.py: 0 of 180); round 4 met the same between torch and the NULL stream on a warm GPU.
                # A stream synchronisation here ends it; the collective hooks below synchronise for the same reason.  (The library's
                # own RCCL path has no hook, and two of its own kernels on one stream have never been seen out of order: every bitwise test.)
                s.synchronize()

        self._hook_keep = GRAD_HOOK(tramp)
        _check(self.L.nrc_cache_set_grad_hook(self.h, self._hook_keep, None))

    def CommStatus(self):
        """nrc_cache_comm_status: raises CommError once the exchange has failed (polls RCCL's asynchronous error state; never blocks)"""
        _check(self.L.nrc_cache_comm_status(self.h))

    def SetCommTimeoutMs(self, ms):
        """deadline of the library's waits behind a collective (default 30 000 ms once the frame has more than one rank; 0: none)"""
        _check(self.L.nrc_cache_set_comm_timeout_ms(self.h, C.c_uint32(int(ms))))

    def SetRawCollectiveHooks(self, rank, world, allreduce, allgather):
        """nrc_cache_set_collective_hooks with the caller's own ALLREDUCE_F64_HOOK / ALLGATHER_HOOK callables (tests: failing transports)"""
        self._coll_keep = (ALLREDUCE_F64_HOOK(allreduce), ALLGATHER_HOOK(allgather))
        _check(self.L.nrc_cache_set_collective_hooks(self.h, C.c_int(rank), C.c_int(world), self._coll_keep[0], self._coll_keep[1], None))

    def SetCollectiveHooks(self, rank, world, group=None):
        """the frame gather / metric reduction of a cache WITHOUT a native RCCL communicator go through torch.distributed (any backend:
        the gloo rehearsals of tests/ stage through host memory).  nrc_cache_set_collective_hooks."""
        import torch
        import torch.distributed as dist

        def on(stream):
            return torch.cuda.stream(torch.cuda.ExternalStream(int(stream or 0)))

        def staged(t):
            if dist.get_backend(group) == "nccl":
                return t
            return t.cpu()      # host-staged transport (the library has waited for its own work on the stream: include/nrc_hpm.h)

        def allreduce(_user, buf, n, stream):
            try:
                with on(stream):
                    t = _wrap_device(buf, int(n) * 8, torch.float64, (int(n),))
                    h = staged(t)
                    dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
                    if h is not t:
                        t.copy_(h)
                        torch.cuda.current_stream().synchronize()
                return 0
            except Exception as e:      # noqa: BLE001 -- a Python exception must not unwind through the C frames
                print("collective hook (all-reduce) failed: %r" % (e,))
                return 1

        def allgather(_user, send, recv, nbytes, stream):
            try:
                with on(stream):
                    s_ = _wrap_device(send, int(nbytes), torch.uint8, (int(nbytes),))
                    r_ = _wrap_device(recv, int(nbytes) * world, torch.uint8, (world, int(nbytes)))
                    if dist.get_backend(group) == "nccl":
                        dist.all_gather_into_tensor(r_.view(-1), s_, group=group)
                    else:
                        parts = [torch.empty(int(nbytes), dtype=torch.uint8) for _ in range(world)]
                        hs = staged(s_)
                        dist.all_gather(parts, hs, group=group)
                        r_.copy_(torch.stack(parts))
                        torch.cuda.current_stream().synchronize()
                return 0
            except Exception as e:      # noqa: BLE001
                print("collective hook (all-gather) failed: %r" % (e,))
                return 1

        self._coll_keep = (ALLREDUCE_F64_HOOK(allreduce), ALLGATHER_HOOK(allgather))
        _check(self.L.nrc_cache_set_collective_hooks(self.h, C.c_int(rank), C.c_int(world), self._coll_keep[0], self._coll_keep[1], None))

    def GetParams(self, which=0):
        out = np.zeros(self.ParamCount(), np.float32)
        _check(self.L.nrc_cache_get_params(self.h, C.c_int(which), out.ctypes.data_as(C.c_void_p)))
        return out

    def SetParams(self, which, values):
        v = np.ascontiguousarray(values, np.float32)
        assert v.size == self.ParamCount()
        _check(self.L.nrc_cache_set_params(self.h, C.c_int(which), v.ctypes.data_as(C.c_void_p)))

    def ParamCountTcnn(self):
        return int(self.L.nrc_cache_param_count_tcnn(self.h))

    def GetParamsTcnn(self, which=0):
        """buffer `which` in tiny-cuda-nn's own layout (output matrix padded to 16 rows): what a weight dump of the reference holds"""
        out = np.zeros(self.ParamCountTcnn(), np.float32)
        _check(self.L.nrc_cache_get_params_tcnn(self.h, C.c_int(which), out.ctypes.data_as(C.c_void_p)))
        return out

    def SetParamsTcnn(self, which, values):
        v = np.ascontiguousarray(values, np.float32)
        assert v.size == self.ParamCountTcnn()
        _check(self.L.nrc_cache_set_params_tcnn(self.h, C.c_int(which), v.ctypes.data_as(C.c_void_p)))

    def SaveCheckpoint(self, path):
        """nrc_cache_save_checkpoint: model shape + step + weights / EMA weights / Adam moments (tiny-cuda-nn layout) in one file"""
        _check(self.L.nrc_cache_save_checkpoint(self.h, os.fsencode(path)))

    def LoadCheckpoint(self, path):
        _check(self.L.nrc_cache_load_checkpoint(self.h, os.fsencode(path)))

    def GetStep(self):
        s = C.c_uint32(0)
        _check(self.L.nrc_cache_get_step(self.h, C.byref(s)))
        return s.value

    def SetStep(self, step):
        _check(self.L.nrc_cache_set_step(self.h, C.c_uint32(step)))

    def state_dict(self):
        """checkpoint (the reference has none): fp32 master/EMA weights + Adam state + step"""
        return dict(step=self.GetStep(), **{k: self.GetParams(i) for i, k in enumerate(("w", "ema", "m", "v"))})

    def load_state_dict(self, sd):
        for i, k in enumerate(("w", "ema", "m", "v")):
            self.SetParams(i, sd[k])
        self.SetStep(int(sd["step"]))

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------------------------
class NrcHpmRenderer(_LiveMedium):
    """en::NrcHpmRenderer (src/NrcHpmRenderer.cu).  `queue` arguments of the reference become the HIP stream."""
    _PREFIX = "nrc_renderer_"
    BUF = dict(primary=0, info=1, origin=2, dir=3, infer_input=4, infer_output=5, train_input=6, train_target=7, ring=8,
               tail_query=9, tail_record=10, tail_output=11, live=12)

    def __init__(self, width, height, blend, camera, appConfig, hpmScene, nrc, tile=None, stream=None):
        self.L = load_library()
        self.width, self.height = width, height
        self.nrc = nrc
        self._scene = make_c_scene(hpmScene)
        cam = make_c_camera(camera)
        t = None
        self.tile = tuple(int(x) for x in tile) if tile is not None else None
        if tile is not None:
            t = NrcTile(*[int(x) for x in tile])
        h = C.c_void_p()
        _check(self.L.nrc_renderer_create(C.c_uint32(width), C.c_uint32(height), C.c_int(int(blend)), C.byref(cam),
                                          C.byref(appConfig.c), C.byref(self._scene), nrc.h,
                                          C.byref(t) if t is not None else None, _stream_ptr(stream), C.byref(h)))
        self.h = h

    def Render(self, queue=None, train=False):
        _check(self.L.nrc_renderer_render(self.h, C.c_int(int(bool(train)))))

    def RenderFrames(self, frameRandoms, train=False):
        """len(frameRandoms) consecutive Render(queue, train) calls enqueued by one call into the library; frameRandoms: [n][4]"""
        r = np.ascontiguousarray(frameRandoms, np.float32).reshape(-1, 4)
        if not hasattr(self.L, "nrc_renderer_render_frames"):      # an older build loaded through NRC_HPM_LIB (A/B tooling)
            for row in r:
                self.SetFrameRandom(row)
                self.Render(None, train)
            return
        _check(self.L.nrc_renderer_render_frames(self.h, C.c_uint32(r.shape[0]), r.ctypes.data_as(C.c_void_p), C.c_int(int(bool(train)))))

    def SetCamera(self, queue, camera):
        cam = make_c_camera(camera)
        _check(self.L.nrc_renderer_set_camera(self.h, C.byref(cam)))

    def RenderPath(self, cameras, framesPerCamera, frameRandoms=None, train=False, out=None):
        """a camera path (include/nrc_hpm.h, nrc_renderer_render_path): for every camera of `cameras` (scene.make_camera / scene.orbit_cameras)
        SetCamera + framesPerCamera Render calls, bit for bit, enqueued by one call that does not wait for the GPU.  Returns the views as a
        torch CUDA tensor [n, height, width, 4] (`out` when given; out=False: no images, the last view stays in GetImage()); the stream given
        at construction is ordered behind the last view's copy.  frameRandoms: None or [n * framesPerCamera][4].
        times: None, or one time per view into the volume keys (SetVolumeKeys): SetVolumeTime(times[i]) in front of view i's SetCamera
        (nrc_renderer_render_path_timed); one time outside [0, VolumeKeyCount() - 1] fails the call before anything is rendered."""
        return self._path(cameras, framesPerCamera, frameRandoms, train, out, None)
    RenderPath = _times_keyword(RenderPath)

    def _path(self, cameras, framesPerCamera, frameRandoms, train, out, times):
        tr = C.c_int(int(bool(train)))

        def call(n, cams, fpc, rnd, img, t=None):
            if t is None:
                return self.L.nrc_renderer_render_path(self.h, n, cams, fpc, rnd, tr, img)
            return self.L.nrc_renderer_render_path_timed(self.h, n, cams, t, fpc, rnd, tr, img)
        return _render_path(call, self.width, self.height, cameras, framesPerCamera, frameRandoms, out, times)

    def SetBlend(self, blend):
        _check(self.L.nrc_renderer_set_blend(self.h, C.c_int(int(blend))))

    def SetShowNrc(self, show):
        _check(self.L.nrc_renderer_set_show_nrc(self.h, C.c_int(int(show))))

    def SetFrameRandom(self, r4):
        r = (C.c_float * 4)(*[float(x) for x in r4])
        _check(self.L.nrc_renderer_set_frame_random(self.h, r))

    def ExportOutputImageToFile(self, queue, filePath, root=0):
        """src/NrcHpmRenderer.cu:437-493.  A sharded renderer (tile of a multi-GPU frame) exports the WHOLE frame: collective over the
        frame's ranks, rank `root` writes the file"""
        if self.tile is not None and self.tile[1] > 1:
            _check(self.L.nrc_renderer_export_exr_gathered(self.h, filePath.encode(), C.c_int(root)))
        else:
            _check(self.L.nrc_renderer_export_exr(self.h, filePath.encode()))

    def SetSchedule(self, camera_priority_low=-1, cost_order_lag=-1, xcd_window=-1, composite_defer=-1):
        """nrc_renderer_set_schedule: pin scheduling knobs (values >= 0) or hand them back to the library's tuner (-1); no knob changes a pixel"""
        v = (C.c_int32 * 4)(int(camera_priority_low), int(cost_order_lag), int(xcd_window), int(composite_defer))
        _check(self.L.nrc_renderer_set_schedule(self.h, v))

    def GetSchedule(self):
        """the schedule in use now: dict(camera_priority_low, cost_order_lag, xcd_window, composite_defer, tuning_done)"""
        v = (C.c_int32 * 4)()
        done = C.c_int(0)
        _check(self.L.nrc_renderer_get_schedule(self.h, v, C.byref(done)))
        d = dict(camera_priority_low=v[0], cost_order_lag=v[1], xcd_window=v[2], composite_defer=v[3], tuning_done=bool(done.value))
        if hasattr(self.L, "nrc_renderer_schedule_source"):
            d["source"] = (self.L.nrc_renderer_schedule_source(self.h) or b"").decode()
            d["key"] = (self.L.nrc_renderer_schedule_key(self.h) or b"").decode()
        return d

    def GatherFrame(self, stream=None):
        """the whole [global_h, global_w, 4] frame of a sharded renderer as a new torch CUDA tensor, on every rank (collective: one
        all-gather through the cache's communicator + a de-interleave kernel); an unsharded renderer returns a copy of its image"""
        import torch
        gw, gh = (self.tile[2], self.tile[3]) if self.tile is not None else (self.width, self.height)
        out = torch.empty((gh, gw, 4), device="cuda", dtype=torch.float32)
        _check(self.L.nrc_renderer_gather_frame(self.h, _dev_ptr(out), _stream_ptr(stream)))
        return out

    def GetFrameTimeMS(self):
        return float(self.L.nrc_renderer_frame_time_ms(self.h, None))

    def EvaluateTimestampQueries(self):
        st = (C.c_float * 8)()
        self.L.nrc_renderer_frame_time_ms(self.h, st)
        names = ("clear", "gen_rays", "prep_infer", "train", "prep_train", "infer", "render", "total")
        return dict(zip(names, [float(x) for x in st]))

    def StageStats(self, reset=True):
        """average per-stage ms over all frames since the last reset (HIP events on the render stream)"""
        st = (C.c_float * 8)()
        n = C.c_uint32(0)
        _check(self.L.nrc_renderer_stage_stats(self.h, st, C.byref(n), C.c_int(int(reset))))
        names = ("clear", "gen_rays", "prep_infer", "train", "prep_train", "infer", "render", "total")
        d = dict(zip(names, [float(x) for x in st]))
        d["frames"] = n.value
        return d

    def FrameTimeline(self, max_frames=4096):
        """[frames, 6] ms from the first frame's start (since the last reset) to each frame's events: gen_rays start / done, train rays
        done, inference done, compositing done, training done (nrc_renderer_frame_timeline)"""
        import numpy as np
        buf = (C.c_float * (6 * max_frames))()
        n = C.c_uint32(0)
        _check(self.L.nrc_renderer_frame_timeline(self.h, buf, C.c_uint32(max_frames), C.byref(n)))
        return np.ctypeslib.as_array(buf)[:6 * n.value].reshape(n.value, 6).copy()

    def ResetStageStats(self):
        """forget the frames rendered so far without reading their events (StageStats(reset=True) reads every one of them first)"""
        _check(self.L.nrc_renderer_stage_stats(self.h, None, None, C.c_int(1)))

    def GetImage(self, stream=None):
        """RGBA32F framebuffer as a torch CUDA tensor view [height, width, 4].  The stream given at construction (default) or
        `stream` (a torch stream / raw handle of the consumer) is ordered behind the frame's compositing."""
        import torch
        if stream is None:
            p = self.L.nrc_renderer_framebuffer(self.h)
        else:
            p = self.L.nrc_renderer_framebuffer_on(self.h, _stream_ptr(stream))
        return _wrap_device(p, self.width * self.height * 16, torch.float32, (self.height, self.width, 4))

    def ReleaseImage(self, stream):
        """the consumer's reads of GetImage(stream) enqueued so far end here; the next frame's compositing waits for them"""
        _check(self.L.nrc_renderer_release_frame(self.h, _stream_ptr(stream)))

    def IsBlending(self):
        return bool(self.L.nrc_renderer_is_blending(self.h))

    def SetStageEvents(self, on=True):
        """per-stage timing events (EvaluateTimestampQueries / StageStats) of every stage (default) or of gen_rays only"""
        _check(self.L.nrc_renderer_set_stage_events(self.h, C.c_int(int(on))))

    def SetEmptySkip(self, on=True):
        """exact empty-space early-out of camera rays (default on); off = every ray is traced"""
        _check(self.L.nrc_renderer_set_empty_skip(self.h, C.c_int(int(on))))

    def SetCostOrder(self, on=True):
        """costliest-first launch order of gen_rays' tiles from earlier frames' per-tile times (default on); frames do not change"""
        _check(self.L.nrc_renderer_set_cost_order(self.h, C.c_int(int(on))))

    def SetHotTiles(self, on=True):
        """start the tiles with a pixel in a capped RNG state first (default on); frames do not change"""
        _check(self.L.nrc_renderer_set_hot_tiles(self.h, C.c_int(int(on))))

    def HotTiles(self):
        """(tiles [(tx, ty), ...] gen_rays started first in the last frame, total count found, computed one frame ahead?) or None"""
        import numpy as np
        out = np.zeros(9, np.uint32)
        rc = self.L.nrc_renderer_hot_tiles(self.h, out.ctypes.data_as(C.c_void_p))
        if rc == -2:
            raise RuntimeError(self.L.nrc_last_error().decode() or "nrc_renderer_hot_tiles failed")
        if rc < 0:
            return None
        n = int(out[8])
        return [(int(t & 0xffff), int(t >> 16)) for t in out[:min(n, 8)]], n, rc == 1

    def TileOrder(self):
        """the tile permutation the next frame launches in (numpy uint32)"""
        import numpy as np
        n = self.L.nrc_renderer_tile_order(self.h, None, C.c_size_t(0))
        out = np.zeros(n, np.uint32)
        got = self.L.nrc_renderer_tile_order(self.h, out.ctypes.data_as(C.c_void_p), C.c_size_t(n))
        if got != n:
            raise RuntimeError(self.L.nrc_last_error().decode() or "nrc_renderer_tile_order failed")
        return out

    def SetFullVertexImages(self, on=True):
        """store nrcRayOrigin / nrcRayDir for every pixel (the reference's images) instead of the train grid's pixels only"""
        _check(self.L.nrc_renderer_set_full_vertex_images(self.h, C.c_int(int(on))))

    def VertexImageBytes(self):
        return int(self.L.nrc_renderer_vertex_image_bytes(self.h))

    def Buffer(self, name):
        import torch
        nbytes = C.c_size_t(0)
        p = self.L.nrc_renderer_buffer(self.h, C.c_int(self.BUF[name]), C.byref(nbytes))
        if not p:
            _check(-1)
        if name in ("ring", "live"):
            return _wrap_device(p, nbytes.value, torch.int32, (nbytes.value // 4,))
        inner = {"primary": 4, "info": 1, "origin": 4, "dir": 4, "infer_input": 5, "infer_output": 3,
                 "train_input": 5, "train_target": 3, "tail_query": 5, "tail_record": 4, "tail_output": 3}[name]
        return _wrap_device(p, nbytes.value, torch.float32, (nbytes.value // (4 * inner), inner))

    def TrainGrid(self):
        o = (C.c_uint32 * 5)()
        _check(self.L.nrc_renderer_train_grid(self.h, o))
        return dict(tw=o[0], th=o[1], x_dist=o[2], y_dist=o[3], ring_size=o[4])

    def CountFetches(self, enable=True):
        v = C.c_ulonglong(0)
        _check(self.L.nrc_renderer_count_fetches(self.h, C.c_int(int(enable)), C.byref(v)))
        return v.value

    def MaskedFetches(self):
        """of the look-ups CountFetches has counted since it was last called, those a dead walk (transmittance exactly 0) kept from memory"""
        v = C.c_ulonglong(0)
        _check(self.L.nrc_renderer_masked_fetches(self.h, C.byref(v)))
        return v.value

    def CutFetches(self):
        """the far cut's proof since CountFetches was last called: (the camera walk's collisions at or behind the cut in waves it applies
        to, those of them that met density -- 0 when the cut is sound)"""
        v = (C.c_ulonglong * 2)()
        _check(self.L.nrc_renderer_cut_fetches(self.h, v))
        return int(v[0]), int(v[1])

    def Destroy(self):
        if self.h:
            _check(self.L.nrc_renderer_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass


class McHpmRenderer(_LiveMedium):
    """en::McHpmRenderer (src/McHpmRenderer.cpp)."""
    _PREFIX = "nrc_mc_renderer_"

    def __init__(self, width, height, pathLength, blend, camera, scene, tile=None, stream=None):
        self.L = load_library()
        self.width, self.height = width, height
        self._scene = make_c_scene(scene)
        cam = make_c_camera(camera)
        t = NrcTile(*[int(x) for x in tile]) if tile is not None else None
        h = C.c_void_p()
        _check(self.L.nrc_mc_renderer_create(C.c_uint32(width), C.c_uint32(height), C.c_uint32(pathLength),
                                             C.c_int(int(blend)), C.byref(cam), C.byref(self._scene),
                                             C.byref(t) if t is not None else None, _stream_ptr(stream), C.byref(h)))
        self.h = h

    def Render(self, queue=None):
        _check(self.L.nrc_mc_renderer_render(self.h))

    def SetCamera(self, queue, camera):
        cam = make_c_camera(camera)
        _check(self.L.nrc_mc_renderer_set_camera(self.h, C.byref(cam)))

    def RenderPath(self, cameras, framesPerCamera, frameRandoms=None, train=False, out=None):
        """see NrcHpmRenderer.RenderPath (this renderer does not train: `train` must be False)"""
        return self._path(cameras, framesPerCamera, frameRandoms, train, out, None)
    RenderPath = _times_keyword(RenderPath)

    def _path(self, cameras, framesPerCamera, frameRandoms, train, out, times):
        if train:
            raise ValueError("McHpmRenderer.RenderPath: the Monte Carlo renderer has nothing to train")

        def call(n, cams, fpc, rnd, img, t=None):
            if t is None:
                return self.L.nrc_mc_renderer_render_path(self.h, n, cams, fpc, rnd, img)
            return self.L.nrc_mc_renderer_render_path_timed(self.h, n, cams, t, fpc, rnd, img)
        return _render_path(call, self.width, self.height, cameras, framesPerCamera, frameRandoms, out, times)

    def SetBlend(self, blend):
        _check(self.L.nrc_mc_renderer_set_blend(self.h, C.c_int(int(blend))))

    def IsBlending(self):
        return bool(self.L.nrc_mc_renderer_is_blending(self.h))

    def SetEmptySkip(self, on=True):
        _check(self.L.nrc_mc_renderer_set_empty_skip(self.h, C.c_int(int(on))))

    def SetCostOrder(self, on=True):
        _check(self.L.nrc_mc_renderer_set_cost_order(self.h, C.c_int(int(on))))

    def SetFrameRandom(self, r4):
        r = (C.c_float * 4)(*[float(x) for x in r4])
        _check(self.L.nrc_mc_renderer_set_frame_random(self.h, r))

    def ExportOutputImageToFile(self, queue, filePath):
        _check(self.L.nrc_mc_renderer_export_exr(self.h, filePath.encode()))

    def GetFrameTimeMS(self):
        return float(self.L.nrc_mc_renderer_frame_time_ms(self.h))

    def GetImage(self):
        import torch
        p = self.L.nrc_mc_renderer_framebuffer(self.h)
        return _wrap_device(p, self.width * self.height * 16, torch.float32, (self.height, self.width, 4))

    def CountFetches(self, enable=True):
        v = C.c_ulonglong(0)
        _check(self.L.nrc_mc_renderer_count_fetches(self.h, C.c_int(int(enable)), C.byref(v)))
        return v.value

    def Destroy(self):
        if self.h:
            _check(self.L.nrc_mc_renderer_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass


def comm_unique_id():
    buf = (C.c_char * 128)()
    _check(load_library().nrc_comm_unique_id(buf))
    return bytes(buf)


def CompareImages(ref, own, stream=None):
    """Reference::Result (include/engine/graphics/Reference.hpp:17-29): torch CUDA RGBA32F [h,w,4] images."""
    r = (C.c_float * 5)()
    h, w = ref.shape[0], ref.shape[1]
    _check(load_library().nrc_compare_images(_dev_ptr(ref), _dev_ptr(own), C.c_uint32(w), C.c_uint32(h),
                                             _stream_ptr(stream), r))
    return dict(mse=r[0], ref_mean=r[1], own_mean=r[2], own_var=r[3], valid=r[4])


def CompareImagesSharded(nrc, ref_local, own_local, stream=None):
    """Reference::Result of a frame sharded over ranks: every rank passes ITS pixels (torch CUDA RGBA32F [h, local_w, 4]) and receives
    the whole frame's metrics -- five local fp64 sums, two small all-reduces through `nrc`'s communicator (collective call)"""
    r = (C.c_float * 5)()
    n = int(ref_local.shape[0]) * int(ref_local.shape[1])
    assert tuple(ref_local.shape) == tuple(own_local.shape) and ref_local.is_contiguous() and own_local.is_contiguous()
    _check(load_library().nrc_compare_images_sharded(nrc.h, _dev_ptr(ref_local), _dev_ptr(own_local), C.c_uint32(n), _stream_ptr(stream), r))
    return dict(mse=r[0], ref_mean=r[1], own_mean=r[2], own_var=r[3], valid=r[4])


def check_guards():
    """NRC_DEBUG=guard_alloc: (number of allocations whose canaries were overwritten, description of the first); (-1, "") when off"""
    buf = C.create_string_buffer(512)
    n = load_library().nrc_debug_check_guards(buf, C.c_size_t(512))
    return int(n), buf.value.decode()


def live_allocations():
    """device allocations the library holds right now (nrc_debug_live_allocations): unchanged by an object's whole life, or a failed creation"""
    return int(load_library().nrc_debug_live_allocations())


def test_math(fn, a, b=None):
    """bit-parity hook: evaluates math-spec function `fn` on the device (torch CUDA float tensors)."""
    import torch
    out, out2 = torch.empty_like(a), torch.empty_like(a)
    _check(load_library().nrc_test_math(C.c_int(fn), _dev_ptr(a), _dev_ptr(b) if b is not None else None,
                                        C.c_uint32(a.numel()), _dev_ptr(out), _dev_ptr(out2), _stream_ptr(None)))
    return out, out2


def test_view_aov_host(scene, camera, width, height, tile=None):
    """nrc_test_view_aov_host: the view AOV [height][width][4] (numpy) of `scene` (scene.make_scene) seen from `camera`, computed on the
    CPU inside the library by csrc/nrc_view_aov.hpp's plain voxel walk; tile: the strip of a sharded frame, as for the renderers"""
    sc_ = make_c_scene(scene.scene if hasattr(scene, "scene") else scene)
    cam = make_c_camera(camera)
    t = NrcTile(*[int(x) for x in tile]) if tile is not None else None
    out = np.empty((height, width, 4), np.float32)
    _check(load_library().nrc_test_view_aov_host(C.byref(sc_), C.byref(cam), C.c_uint32(width), C.c_uint32(height),
                                                 C.byref(t) if t is not None else None, out.ctypes.data_as(C.c_void_p)))
    return out


def camera_rays(camera, width, height, tile=None):
    """nrc_camera_rays: the records {pos, 0, dir, +inf} [height][width][8] (numpy) of the camera rays a renderer of width x height pixels
    walks for its view AOV (unit directions); tile: the strip of a sharded frame.  Host only: no renderer, no GPU."""
    cam = make_c_camera(camera)
    t = NrcTile(*[int(x) for x in tile]) if tile is not None else None
    out = np.empty((height, width, 8), np.float32)
    _check(load_library().nrc_camera_rays(C.byref(cam), C.c_uint32(width), C.c_uint32(height), C.byref(t) if t is not None else None,
                                          out.ctypes.data_as(C.c_void_p)))
    return out


def ortho_rays(view, width, height):
    """nrc_ortho_rays: the same records [height][width][8] of an orthographic view {origin, du, dv, dir} (scene.light_view)"""
    v = make_c_ortho_view(view)
    out = np.empty((height, width, 8), np.float32)
    _check(load_library().nrc_ortho_rays(C.byref(v), C.c_uint32(width), C.c_uint32(height), out.ctypes.data_as(C.c_void_p)))
    return out


def test_ray_aov_host(scene, rays):
    """nrc_test_ray_aov_host: the ray AOV [...][4] (numpy) of the records rays [...][8] through `scene` (scene.make_scene), computed on the
    CPU inside the library by csrc/nrc_view_aov.hpp's plain range walk"""
    sc_ = make_c_scene(scene.scene if hasattr(scene, "scene") else scene)
    r = np.ascontiguousarray(rays, np.float32)
    if r.ndim < 1 or r.shape[-1] != 8:
        raise ValueError("test_ray_aov_host: rays must have 8 numbers per record")
    out = np.empty(r.shape[:-1] + (4,), np.float32)
    n = r.size // 8
    _check(load_library().nrc_test_ray_aov_host(C.byref(sc_), C.c_size_t(n), r.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def deep_ray_aov_host(scene, rays, levels):
    """nrc_test_deep_ray_aov_host: (planes [K][...], flat [...][4]) (numpy) of the records rays [...][8] through `scene`, computed on the CPU
    inside the library by csrc/nrc_view_aov.hpp's plain deep range walk.  The levels go to the library as given: it refuses a bad set."""
    sc_ = make_c_scene(scene.scene if hasattr(scene, "scene") else scene)
    r = np.ascontiguousarray(rays, np.float32)
    if r.ndim < 1 or r.shape[-1] != 8:
        raise ValueError("deep_ray_aov_host: rays must have 8 numbers per record")
    lv = np.ascontiguousarray(np.asarray(levels, np.float32).reshape(-1))
    k, n = int(lv.size), r.size // 8
    z = np.empty((k,) + r.shape[:-1], np.float32)
    flat = np.empty(r.shape[:-1] + (4,), np.float32)
    _check(load_library().nrc_test_deep_ray_aov_host(C.byref(sc_), C.c_size_t(n), r.ctypes.data_as(C.c_void_p), C.c_uint32(k),
                                                     lv.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p)))
    return z, flat


def test_rng(u, v, frame_random, n):
    import torch
    out = torch.zeros(n + 1, device="cuda")
    fr = (C.c_float * 4)(*[float(x) for x in frame_random])
    _check(load_library().nrc_test_rng(C.c_float(u), C.c_float(v), fr, C.c_uint32(n), _dev_ptr(out), _stream_ptr(None)))
    return out


FLIGHT_STATES = 1 << 23
FLIGHT_BITS_SENTINEL = 0xA5C3F00D


def test_flight_select(lambda_, want_table=False, buffers=None):
    """nrc_test_flight_select: the capped-state selection skip_setup makes at `lambda_`, from the free-flight table the renderers read.
    Returns (count, list, bits, slack[, table]) as numpy arrays: list = the 8 words behind the count as the device left them, bits = the
    2^18 words, slack = the two words behind them (filled with FLIGHT_BITS_SENTINEL before the call: the kernel must leave them), table =
    the 2^23 floats when want_table.  buffers: a pair (count_and_list, bits) of torch CUDA int32 tensors of 9 and 2^18 + 2 words to reuse
    (as a renderer reuses its own from one medium to the next); fresh ones, filled with the sentinel, otherwise."""
    import torch
    n_words = FLIGHT_STATES // 32
    if buffers is None:
        fill = FLIGHT_BITS_SENTINEL - (1 << 32)
        buffers = (torch.full((9,), fill, dtype=torch.int32, device="cuda"), torch.full((n_words + 2,), fill, dtype=torch.int32, device="cuda"))
    sel, bits = buffers
    assert sel.numel() == 9 and bits.numel() == n_words + 2 and sel.dtype == torch.int32 and bits.dtype == torch.int32
    table = torch.empty(FLIGHT_STATES, dtype=torch.float32, device="cuda") if want_table else None
    _check(load_library().nrc_test_flight_select(C.c_float(float(lambda_)), _dev_ptr(table) if want_table else None, _dev_ptr(sel), _dev_ptr(bits),
                                                 _stream_ptr(None)))
    torch.cuda.synchronize()
    h_sel = sel.cpu().numpy().view(np.uint32)
    h_bits = bits.cpu().numpy().view(np.uint32)
    out = (int(h_sel[0]), h_sel[1:].copy(), h_bits[:n_words].copy(), h_bits[n_words:].copy())
    return out + (table.cpu().numpy(),) if want_table else out
