"""ctypes binding of libsps_hip.so (C ABI: include/sps_hip.h).

The product path has NO fallback: if the library is missing or fails to load, importing
this module raises.  Device pointers are passed as integers (``tensor.data_ptr()``)."""
from __future__ import annotations

import ctypes as C
import os

from . import _build

NUM_LEVELS = 5
SPS_OK = 0
ERR_RANGE = -4
ERR_NOMEM = -3
ERR_INVALID = -1
ERR_ITEMCAP = -6


class SpsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libsps_hip error {code}: {msg}")
        self.code = code


ABI_VERSION = 202          # sps_version() of the library this binding was written against


def _load() -> C.CDLL:
    # SPS_LIB: diagnostic builds (tools/ablate*.sh, tune_conv.sh ...) live at their own path and never overwrite
    # the product library
    path = os.environ.get("SPS_LIB") or _build.LIB
    if path == _build.LIB and (not os.path.exists(path) or _build.is_stale()):
        # an edited .hip / .inc.h must never run against an old binary: rebuild when hipcc is here (it cross-compiles
        # without a GPU); a box without hipcc runs the shipped .so, whose ABI version is checked below.
        # Never falls back to CPU code.
        if _build.have_hipcc():
            path = _build.build()
        elif not os.path.exists(path):
            raise ImportError("libsps_hip.so is missing and hipcc is not available to build it")
    # One HIP runtime per process: PyTorch ships its own libamdhip64 / libhsa-runtime64.  Loaded AFTER torch, this library binds
    # to the copies torch already mapped (same SONAME); loaded BEFORE it, /opt/rocm's copies come in first and the process ends
    # up with two runtimes, of which the second finds "no ROCm-capable device" (seen with __graft_entry__.build() followed by
    # smoke() in one process).  The host side of this package is PyTorch's anyway (device memory, streams).
    import importlib.util
    if importlib.util.find_spec("torch") is not None:     # (the ctypes binding alone works without torch)
        import torch  # noqa: F401
    lib = C.CDLL(path)
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float
    sig = {
        "sps_last_error": (C.c_char_p, []),
        "sps_version": (i32, []),
        "sps_ctx_create": (i32, [i32, C.POINTER(vp)]),
        "sps_ctx_destroy": (i32, [vp]),
        "sps_reserve": (i32, [vp, i64]),
        "sps_ctx_set_level_fractions": (i32, [vp, vp]),
        "sps_ctx_set_inference_only": (i32, [vp, i32]),
        "sps_ctx_set_pipelined": (i32, [vp, i32]),
        "sps_arena_bytes": (i64, [vp]),
        "sps_weights_num_tensors": (i32, []),
        "sps_weights_tensor_info": (i32, [i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i64)]),
        "sps_weights_numel": (i64, []),
        "sps_weights_load": (i32, [vp, vp, i64]),
        "sps_weights_create": (i32, [i32, vp, i64, i32, C.POINTER(vp)]),
        "sps_weights_destroy": (i32, [vp]),
        "sps_ctx_set_weights": (i32, [vp, vp]),
        "sps_forward": (i32, [vp, vp, i64, i64, f32, vp, vp]),
        "sps_forward_metrics": (i32, [vp, vp, i64, i64, f32, f32, i32, vp, vp, vp]),
        "sps_head_num_tensors": (i32, [i32]),
        "sps_head_tensor_info": (i32, [i32, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i64)]),
        "sps_head_numel": (i64, [i32]),
        "sps_weights_load_head": (i32, [vp, vp, i64, i32]),
        "sps_forward_head": (i32, [vp, vp, i64, i64, f32, vp, f32, vp, i64, i32, vp]),
        "sps_check": (i32, [vp, vp]),
        "sps_metrics": (i32, [vp, vp, vp, i64, i64, f32, i32, C.POINTER(C.c_double), vp]),
        "sps_metrics_dev": (i32, [vp, vp, vp, i64, i64, f32, i32, vp, vp]),
        "sps_profile_enable": (i32, [vp, i32]),
        "sps_profile_count": (i32, [vp]),
        "sps_profile_read": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(f32)]),
        "sps_profile_kernel": (i32, [vp, i32, C.c_char_p, i32]),
        "sps_map_upload": (i32, [vp, vp, i64, i64, f32, vp]),
        "sps_map_upload_voxels": (i32, [vp, vp, i64, i64, vp]),
        "sps_submap_voxel": (i32, [vp, vp, i64, i64, vp, C.POINTER(i64), C.POINTER(i64), vp]),
        "sps_submap_voxel_ijk": (i32, [vp, vp, i64, i64, f32, vp, C.POINTER(i64), C.POINTER(i64), vp]),
        "sps_transform_points": (i32, [vp, vp, i32, i64, i64, vp, vp, i32, i64, vp]),
        "sps_filter_prepare": (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp]),
        "sps_forward_n": (i32, [vp, vp, i64, i64, vp, f32, vp, vp]),
        "sps_compact_stable": (i32, [vp, vp, vp, i64, i32, i64, f32, vp, vp, vp]),
        "sps_filter_finish": (i32, [vp, vp, i64, vp, i64, i32, i32, vp, vp, f32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "sps_train_forward": (i32, [vp, vp, i64, vp, i64, i64, f32, vp, vp, vp]),
        "sps_train_backward": (i32, [vp, vp, vp, vp, i64, vp]),
        "sps_train_generation": (i32, [vp, C.POINTER(i64)]),
        "sps_train_wgrad_plan": (i32, [vp, C.c_char_p, C.POINTER(i32), C.POINTER(i32)]),
        "sps_train_backward_at": (i32, [vp, i64, vp, vp, vp, i64, vp]),
        "sps_scan_mse": (i32, [vp, vp, i64, vp, i64, i64, vp, vp, vp]),
        "sps_scan_mse_backward": (i32, [vp, vp, i64, vp, i64, i64, vp, vp, vp, vp]),
        "sps_radius_grid_upload": (i32, [vp, vp, vp, vp, vp, i64, i64, C.c_double, C.c_double, vp]),
        "sps_radius_count": (i32, [vp, vp, i64, i64, vp, vp]),
        "sps_radius_fill": (i32, [vp, vp, i64, i64, vp, vp, vp]),
        "sps_radius_grid_attach": (i32, [vp, vp]),
        "sps_radius_item": (i32, [vp, vp, i32, i64, i64, f32, vp, vp, i64, i64, vp, vp]),
        "sps_forward_metrics_n": (i32, [vp, vp, i64, i64, vp, f32, f32, i32, vp, vp, vp]),
        "sps_level_counts": (i32, [vp, C.POINTER(i64)]),
        "sps_get_voxels": (i32, [vp, i32, vp]),
        "sps_get_block_slots": (i32, [vp, i32, C.POINTER(i64), C.POINTER(i64), vp, i64]),
        "sps_get_inverse": (i32, [vp, vp]),
        "sps_get_parent": (i32, [vp, i32, vp]),
        "sps_get_map_pairs": (i32, [vp, i32, C.POINTER(i64)]),
        "sps_get_tile_masks": (i32, [vp, i32, vp, C.POINTER(i64)]),
        "sps_get_nbr": (i32, [vp, i32, vp]),
        "sps_get_kernel_map": (i32, [vp, i32, i32, vp, C.POINTER(i64)]),
        "sps_get_rulebook_chunks": (i32, [vp, i32, vp, C.POINTER(i64)]),
        "sps_get_conv_launch": (i32, [vp, C.c_char_p, C.POINTER(i32)]),
        "sps_get_logits": (i32, [vp, vp]),
        "sps_get_feature": (i32, [vp, C.c_char_p, vp, C.POINTER(i64), C.POINTER(i64)]),
        "sps_lts_num_tensors": (i32, []),
        "sps_lts_tensor_info": (i32, [i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]),
        "sps_lts_numel": (i64, []),
        "sps_lts_lidar_info": (i32, [i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "sps_lts_create": (i32, [i32, vp, i64, C.POINTER(vp)]),
        "sps_lts_destroy": (i32, [vp]),
        "sps_lts_project": (i32, [vp, vp, i64, i64, i32, vp, vp, vp, vp]),
        "sps_lts_forward": (i32, [vp, vp, i64, i64, vp, vp]),
        "sps_lts_check": (i32, [vp, vp]),
        "sps_lts_tap": (i32, [vp, i32, vp, C.POINTER(i64), C.POINTER(i64), vp]),
        "sps_forward_head_n": (i32, [vp, vp, i64, i64, vp, f32, vp, f32, vp, i64, i32, vp]),
        "sps_transform_rows": (i32, [vp, vp, i32, i64, i64, vp, f32, vp, i64, vp, f32, vp]),
        "sps_transform_points_n": (i32, [vp, vp, i32, i64, i64, vp, vp, vp, i32, i64, vp]),
        "sps_radius_crop": (i32, [vp, vp, i32, i64, i64, vp, C.c_double, vp, i64, vp, i64, i64, vp, f32, vp, vp]),
        "sps_label_filter": (i32, [vp, vp, i64, i64, vp, i64, vp, i64, vp, vp, vp, vp]),
        "sps_loc_downsample_scratch": (i64, [i64]),
        "sps_loc_align_scratch": (i64, [i64]),
        "sps_loc_downsample": (i32, [vp, vp, i64, i64, vp, C.c_double, vp, i64, vp, vp, vp]),
        "sps_loc_align": (i32, [vp, vp, vp, i64, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]),
        "sps_loc_match_status_scratch": (i64, [i64]),
        "sps_loc_match_status": (i32, [vp, vp, vp, i64, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, i32, vp, vp, vp,
                                       vp]),
        "sps_ndt_align_scratch": (i64, [i64]),
        "sps_ndt_map_build": (i32, [vp, vp, vp, vp, vp, i64, i64, C.c_double, i32, C.c_double, vp]),
        "sps_ndt_map_cells": (i32, [vp, vp, vp, vp, vp, vp]),
        "sps_ndt_align": (i32, [vp, vp, vp, i64, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp,
                                vp]),
        "sps_ndt_align_batch_scratch": (i64, [i64, i32]),
        "sps_ndt_align_batch": (i32, [vp, vp, vp, i64, vp, i32, i32, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp,
                                      vp, vp, vp, vp, vp]),
        "sps_ndt_score_scratch": (i64, [i64, i64]),
        "sps_ndt_score_poses": (i32, [vp, vp, vp, i64, vp, i64, i32, C.c_double, vp, vp, vp]),
        "sps_ndt_top_poses": (i32, [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp]),
        "sps_bbs_map_build": (i32, [vp, vp, i64, i64, i32, vp]),
        "sps_bbs_map_level": (i32, [vp, i32, vp]),
        "sps_bbs_search_scratch": (i64, [i64, i64, i64]),
        "sps_bbs_search": (i32, [vp, vp, vp, i64, vp, C.c_double, i64, i64, C.c_double, C.c_double, vp, i64, i64, i32, i32, vp, vp,
                                 vp, vp, vp, vp, vp, vp]),
        "sps_ndt_map_build_dynamic": (i32, [vp, vp, vp, vp, vp, i64, i64, C.c_double, i32, C.c_double, i64, vp]),
        "sps_ndt_map_update_scratch": (i64, [i64]),
        "sps_ndt_map_update": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, vp, vp, vp]),
        "sps_ndt_map_info": (i32, [vp, vp]),
        "sps_ndt_map_carve_scratch": (i64, [i64]),
        "sps_ndt_map_carve": (i32, [vp, vp, vp, i64, vp, vp, vp, C.c_double, C.c_double, i32, i32, i32, vp, vp, vp]),
        "sps_ndt_map_carve_cells": (i32, [vp, vp, vp, vp]),
        "sps_ndt_pyramid_build": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i64, i32, C.c_double, C.c_double, vp]),
        "sps_ndt_pyramid_cells": (i32, [vp, i32, vp, vp, vp, vp, vp]),
        "sps_ndt_pyramid_align_scratch": (i64, [i64]),
        "sps_ndt_pyramid_align": (i32, [vp, vp, vp, i64, vp, i32, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp,
                                        vp]),
        "sps_ndt_pyramid_build_dynamic": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i64, i32, C.c_double, C.c_double, vp, vp]),
        "sps_ndt_pyramid_update_scratch": (i64, [i64, i32]),
        "sps_ndt_pyramid_update": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, vp, vp, vp]),
        "sps_ndt_pyramid_carve_scratch": (i64, [i64, i32]),
        "sps_ndt_pyramid_carve": (i32, [vp, vp, vp, i64, vp, vp, vp, vp, C.c_double, i32, i32, i32, vp, vp, vp]),
        "sps_ndt_pyramid_info": (i32, [vp, i32, vp]),
        "sps_ndt_pyramid_carve_cells": (i32, [vp, i32, vp, vp, vp]),
        "sps_ndt_pyramid_align_batch_scratch": (i64, [i64, i32]),
        "sps_ndt_pyramid_align_batch": (i32, [vp, vp, vp, i64, vp, i32, i32, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp,
                                              vp, vp, vp, vp, vp, vp]),
        "sps_ndt_source_scratch": (i64, [i64]),
        "sps_ndt_source_build": (i32, [vp, vp, vp, i64, C.c_double, i32, C.c_double, vp, vp, vp, vp, vp]),
        "sps_ndt_align_d2d_scratch": (i64, [i64]),
        "sps_ndt_align_d2d": (i32, [vp, vp, vp, i64, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp,
                                    vp]),
        "sps_ndt_align_d2d_batch_scratch": (i64, [i64, i32]),
        "sps_ndt_align_d2d_batch": (i32, [vp, vp, vp, i64, vp, i32, i32, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp,
                                          vp, vp, vp, vp, vp, vp]),
        "sps_ndt_pyramid_source_scratch": (i64, [i64, i32]),
        "sps_ndt_pyramid_source_build": (i32, [vp, vp, vp, i64, i32, vp, vp, C.c_double, vp, vp, vp, vp, vp]),
        "sps_ndt_pyramid_align_d2d_scratch": (i64, [i64]),
        "sps_ndt_pyramid_align_d2d": (i32, [vp, vp, vp, i64, vp, i32, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp,
                                            vp]),
        "sps_ndt_pyramid_align_d2d_batch_scratch": (i64, [i64, i32]),
        "sps_ndt_pyramid_align_d2d_batch": (i32, [vp, vp, vp, i64, vp, i32, i32, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp,
                                                  vp, vp, vp, vp, vp, vp, vp]),
        "sps_ndt_score_d2d_scratch": (i64, [i64, i64]),
        "sps_ndt_score_poses_d2d": (i32, [vp, vp, vp, i64, vp, i64, i32, C.c_double, vp, vp, vp]),
        "sps_ukf_state_bytes": (i64, []),
        "sps_ukf_init": (i32, [vp, vp, vp, vp, vp]),
        "sps_ukf_predict": (i32, [vp, vp, i32, vp, vp, vp, vp]),
        "sps_ukf_predict_dt": (i32, [vp, C.c_double, vp, vp, vp, vp]),
        "sps_ukf_correct": (i32, [vp, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.sps_version() != ABI_VERSION:
        raise ImportError(f"{path} reports ABI version {lib.sps_version()}, this binding needs {ABI_VERSION}: rebuild it "
                          "(python -m sps_amd._build)")
    return lib


lib = _load()
EXPORTS = ["sps_last_error", "sps_version", "sps_ctx_create", "sps_ctx_destroy", "sps_reserve",
           "sps_ctx_set_level_fractions", "sps_ctx_set_inference_only", "sps_ctx_set_pipelined", "sps_arena_bytes",
           "sps_weights_num_tensors", "sps_weights_tensor_info", "sps_weights_numel", "sps_weights_load",
           "sps_weights_create", "sps_weights_destroy", "sps_ctx_set_weights",
           "sps_forward", "sps_forward_metrics", "sps_head_num_tensors", "sps_head_tensor_info", "sps_head_numel", "sps_weights_load_head",
           "sps_forward_head", "sps_check", "sps_metrics", "sps_metrics_dev",
           "sps_profile_enable", "sps_profile_count", "sps_profile_read", "sps_profile_kernel", "sps_map_upload", "sps_map_upload_voxels",
           "sps_submap_voxel", "sps_submap_voxel_ijk", "sps_transform_points", "sps_filter_prepare", "sps_forward_n",
           "sps_compact_stable", "sps_filter_finish", "sps_train_forward", "sps_train_backward", "sps_train_generation", "sps_train_wgrad_plan", "sps_train_backward_at", "sps_scan_mse", "sps_scan_mse_backward", "sps_radius_grid_upload", "sps_radius_count",
           "sps_radius_fill", "sps_radius_grid_attach", "sps_radius_item", "sps_forward_metrics_n", "sps_level_counts", "sps_get_voxels",
           "sps_get_block_slots", "sps_get_inverse", "sps_get_parent", "sps_get_map_pairs", "sps_get_tile_masks", "sps_get_nbr", "sps_get_kernel_map", "sps_get_rulebook_chunks", "sps_get_conv_launch", "sps_get_logits", "sps_get_feature",
           "sps_lts_num_tensors", "sps_lts_tensor_info", "sps_lts_numel", "sps_lts_lidar_info", "sps_lts_create",
           "sps_lts_destroy", "sps_lts_project", "sps_lts_forward", "sps_lts_check", "sps_lts_tap",
           "sps_forward_head_n", "sps_transform_rows", "sps_transform_points_n", "sps_radius_crop", "sps_label_filter",
           "sps_loc_downsample_scratch", "sps_loc_align_scratch", "sps_loc_downsample", "sps_loc_align",
           "sps_loc_match_status_scratch", "sps_loc_match_status",
           "sps_ndt_align_scratch", "sps_ndt_map_build", "sps_ndt_map_cells", "sps_ndt_align",
           "sps_ndt_align_batch_scratch", "sps_ndt_align_batch",
           "sps_ndt_score_scratch", "sps_ndt_score_poses", "sps_ndt_top_poses",
           "sps_bbs_map_build", "sps_bbs_map_level", "sps_bbs_search_scratch", "sps_bbs_search",
           "sps_ndt_map_build_dynamic", "sps_ndt_map_update_scratch", "sps_ndt_map_update", "sps_ndt_map_info",
           "sps_ndt_map_carve_scratch", "sps_ndt_map_carve", "sps_ndt_map_carve_cells",
           "sps_ndt_pyramid_build", "sps_ndt_pyramid_cells", "sps_ndt_pyramid_align_scratch", "sps_ndt_pyramid_align",
           "sps_ndt_pyramid_build_dynamic", "sps_ndt_pyramid_update_scratch", "sps_ndt_pyramid_update",
           "sps_ndt_pyramid_carve_scratch", "sps_ndt_pyramid_carve", "sps_ndt_pyramid_info", "sps_ndt_pyramid_carve_cells",
           "sps_ndt_pyramid_align_batch_scratch", "sps_ndt_pyramid_align_batch",
           "sps_ndt_source_scratch", "sps_ndt_source_build", "sps_ndt_align_d2d_scratch", "sps_ndt_align_d2d",
           "sps_ndt_align_d2d_batch_scratch", "sps_ndt_align_d2d_batch", "sps_ndt_score_d2d_scratch", "sps_ndt_score_poses_d2d",
           "sps_ndt_pyramid_source_scratch", "sps_ndt_pyramid_source_build", "sps_ndt_pyramid_align_d2d_scratch",
           "sps_ndt_pyramid_align_d2d", "sps_ndt_pyramid_align_d2d_batch_scratch", "sps_ndt_pyramid_align_d2d_batch",
           "sps_ukf_state_bytes", "sps_ukf_init", "sps_ukf_predict", "sps_ukf_predict_dt", "sps_ukf_correct"]
NDT_SRC_REC = 10           # SPS_NDT_SRC_REC: doubles of a source record
BBS_MAX_LEVELS = 8         # SPS_BBS_MAX_LEVELS
BBS_MAX_YAWS = 4096        # SPS_BBS_MAX_YAWS
BBS_MAX_FRONTIER = 65536   # SPS_BBS_MAX_FRONTIER
BBS_INFO_WORDS = 20        # SPS_BBS_INFO_WORDS
BBS_MAX_STORE = 16384      # W + 2^levels - 1 and H + 2^levels - 1 of sps_bbs_map_build stay within this
BBS_MAX_POINTS = 65536     # cap of sps_bbs_search
UKF_MAX_IMU = 256          # SPS_UKF_MAX_IMU
CROP_BLOCK = 1024          # SPS_CROP_BLOCK: map rows per int of sps_radius_crop's scratch


def check(rc: int) -> None:
    if rc != SPS_OK:
        raise SpsError(rc, lib.sps_last_error().decode())


_LAYOUTS: dict = {}


def weight_layout(out_channels: int = 1):
    """((name, offset, numel), ...) of the weight blob, from the library itself (asked once per head width)."""
    cached = _LAYOUTS.get(out_channels)
    if cached is not None:
        return cached
    out = []
    buf = C.create_string_buffer(128)
    off, num = C.c_int64(), C.c_int64()
    n = lib.sps_head_num_tensors(out_channels)
    if n < 0:
        check(n)
    for i in range(n):
        check(lib.sps_head_tensor_info(out_channels, i, buf, 128, C.byref(off), C.byref(num)))
        out.append((buf.value.decode(), off.value, num.value))
    _LAYOUTS[out_channels] = tuple(out)
    return _LAYOUTS[out_channels]


class Weights:
    """One device-resident weight set (sps_weights_create): uploaded once per device and parameter version, attached
    to any number of contexts of that device in O(1)."""

    def __init__(self, device: int, blob_host_ptr: int, numel: int, out_channels: int = 1):
        h = C.c_void_p()
        check(lib.sps_weights_create(int(device), blob_host_ptr, int(numel), int(out_channels), C.byref(h)))
        self.handle = h
        self.device = int(device)

    def close(self):
        if getattr(self, "handle", None):
            lib.sps_weights_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Owns one ``sps_ctx`` (one per process, device and stream)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib.sps_ctx_create(device, C.byref(h)))
        self.handle = h
        self.device = device
        self.weights = None

    def close(self):
        if getattr(self, "handle", None):
            lib.sps_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- thin wrappers ----------------------------------------------------------------
    def reserve(self, max_points: int):
        check(lib.sps_reserve(self.handle, int(max_points)))

    LIDAR_FRACTIONS = (1.0, 0.6, 0.3, 0.15, 0.08)      # V_l / V_0 of 0.1 m LiDAR clouds is ~0.39 / 0.14 / 0.05 / 0.015

    def set_level_fractions(self, frac=None):
        """Compact arena (include/sps_hip.h): level l holds frac[l] * max_points rows; None = full size (never overflows)."""
        arr = None if frac is None else (C.c_float * NUM_LEVELS)(*[float(x) for x in frac])
        check(lib.sps_ctx_set_level_fractions(self.handle, arr))

    def set_inference_only(self, on: bool = True):
        """Inference-only context (include/sps_hip.h): at the pair-exact levels the rulebook replaces the neighbour table
        (less arena, fewer bytes written per scan); training on the context switches it back."""
        check(lib.sps_ctx_set_inference_only(self.handle, 1 if on else 0))

    def set_pipelined(self, on: bool = True):
        """Launch-geometry hint (include/sps_hip.h): True = forwards of several contexts run beside each other (least work per
        forward), False (default) = one forward after another (shortest chain).  Results are bit-identical either way."""
        check(lib.sps_ctx_set_pipelined(self.handle, 1 if on else 0))

    def arena_bytes(self) -> int:
        return int(lib.sps_arena_bytes(self.handle))

    def load_weights(self, blob_host_ptr: int, numel: int, out_channels: int = 1):
        check(lib.sps_weights_load_head(self.handle, blob_host_ptr, int(numel), int(out_channels)))
        self.weights = None

    def set_weights(self, weights: "Weights"):
        check(lib.sps_ctx_set_weights(self.handle, weights.handle))
        self.weights = weights          # keeps the Python owner alive as long as the context uses it

    def forward_head(self, coords_ptr: int, ld: int, n: int, voxel_size: float, feats_ptr, t_base: float,
                     out_ptr: int, ldo: int, activation: int, stream: int):
        check(lib.sps_forward_head(self.handle, coords_ptr, ld, n, voxel_size, feats_ptr, t_base, out_ptr, ldo,
                                   activation, stream))

    def forward_head_n(self, coords_ptr: int, ld: int, n_max: int, n_dev_ptr: int, voxel_size: float, feats_ptr,
                       t_base: float, out_ptr: int, ldo: int, activation: int, stream: int):
        check(lib.sps_forward_head_n(self.handle, coords_ptr, ld, n_max, n_dev_ptr, voxel_size, feats_ptr, t_base, out_ptr,
                                     ldo, activation, stream))

    def forward_metrics(self, batch_ptr: int, ld: int, n: int, voxel_size: float, eps: float, n_batches: int,
                        scores_ptr: int, out_ptr: int, stream: int):
        check(lib.sps_forward_metrics(self.handle, batch_ptr, ld, n, voxel_size, eps, n_batches, scores_ptr, out_ptr, stream))

    def forward_metrics_n(self, batch_ptr: int, ld: int, n_max: int, n_dev_ptr: int, voxel_size: float, eps: float,
                          n_batches: int, scores_ptr: int, out_ptr: int, stream: int):
        check(lib.sps_forward_metrics_n(self.handle, batch_ptr, ld, n_max, n_dev_ptr, voxel_size, eps, n_batches, scores_ptr,
                                        out_ptr, stream))

    def radius_grid_attach(self, owner: "Context"):
        check(lib.sps_radius_grid_attach(self.handle, owner.handle))
        self._grid_owner = owner        # the owner keeps the device copies: it must outlive this view

    def radius_item(self, scan_ptr: int, in_f64: bool, ld: int, n: int, batch_index: float, row_off_ptr, rows_ptr: int,
                    ldo: int, row_cap: int, n_rows_ptr: int, stream: int):
        check(lib.sps_radius_item(self.handle, scan_ptr, int(in_f64), ld, n, float(batch_index), row_off_ptr, rows_ptr, ldo,
                                  row_cap, n_rows_ptr, stream))

    def forward(self, coords_ptr: int, ld: int, n: int, voxel_size: float, scores_ptr: int, stream: int):
        check(lib.sps_forward(self.handle, coords_ptr, ld, n, voxel_size, scores_ptr, stream))

    def check_errors(self, stream: int):
        check(lib.sps_check(self.handle, stream))

    def metrics(self, scores_ptr: int, batch_ptr: int, ld: int, n: int, eps: float, n_batches: int, stream: int):
        out = (C.c_double * (8 * n_batches))()
        check(lib.sps_metrics(self.handle, scores_ptr, batch_ptr, ld, n, eps, n_batches, out, stream))
        return [list(out[8 * b: 8 * b + 8]) for b in range(n_batches)]

    def metrics_dev(self, scores_ptr: int, batch_ptr: int, ld: int, n: int, eps: float, n_batches: int,
                    out_ptr: int, stream: int):
        check(lib.sps_metrics_dev(self.handle, scores_ptr, batch_ptr, ld, n, eps, n_batches, out_ptr, stream))

    def profile_enable(self, on: bool):
        check(lib.sps_profile_enable(self.handle, 1 if on else 0))

    def profile_read(self):
        """[(stage name, milliseconds)] of the last forward (synchronises on the stage events)."""
        out = []
        buf = C.create_string_buffer(96)
        ms = C.c_float()
        for i in range(lib.sps_profile_count(self.handle)):
            check(lib.sps_profile_read(self.handle, i, buf, 96, C.byref(ms)))
            out.append((buf.value.decode(), ms.value))
        return out

    def profile_kernels(self):
        """[kernel class] of the stages profile_read() lists (sps_profile_kernel)."""
        buf = C.create_string_buffer(128)
        out = []
        for i in range(lib.sps_profile_count(self.handle)):
            check(lib.sps_profile_kernel(self.handle, i, buf, 128))
            out.append(buf.value.decode())
        return out

    def map_upload(self, xyz_ptr: int, ld: int, m: int, ds: float, stream: int):
        check(lib.sps_map_upload(self.handle, xyz_ptr, ld, m, ds, stream))

    def map_upload_voxels(self, ijk_ptr: int, ld: int, m: int, stream: int):
        check(lib.sps_map_upload_voxels(self.handle, ijk_ptr, ld, m, stream))

    def submap_voxel(self, scan_ptr: int, ld: int, n: int, out_ptr: int, stream: int):
        a, b = C.c_int64(), C.c_int64()
        check(lib.sps_submap_voxel(self.handle, scan_ptr, ld, n, out_ptr, C.byref(a), C.byref(b), stream))
        return a.value, b.value

    def submap_voxel_ijk(self, scan_ptr: int, ld: int, n: int, ds: float, out_ptr: int, stream: int):
        a, b = C.c_int64(), C.c_int64()
        check(lib.sps_submap_voxel_ijk(self.handle, scan_ptr, ld, n, ds, out_ptr, C.byref(a), C.byref(b), stream))
        return a.value, b.value

    @staticmethod
    def _mat(T):
        """4x4 host matrix -> ctypes double[16] (row-major), None = identity."""
        if T is None:
            return None
        import numpy as np
        a = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(16))
        return (C.c_double * 16)(*a.tolist())

    def transform_points(self, xyz_ptr: int, in_f64: bool, ld: int, n: int, T, out_ptr: int, out_f64: bool, ldo: int,
                         stream: int):
        check(lib.sps_transform_points(self.handle, xyz_ptr, int(in_f64), ld, n, self._mat(T), out_ptr, int(out_f64), ldo,
                                       stream))

    def filter_prepare(self, raw_ptr: int, in_f64: bool, ld: int, n: int, T, batch_ptr: int, counts_ptr: int, stream: int):
        check(lib.sps_filter_prepare(self.handle, raw_ptr, int(in_f64), ld, n, self._mat(T), batch_ptr, counts_ptr, stream))

    def forward_n(self, coords_ptr: int, ld: int, n_max: int, n_dev_ptr: int, voxel_size: float, scores_ptr: int, stream: int):
        check(lib.sps_forward_n(self.handle, coords_ptr, ld, n_max, n_dev_ptr, voxel_size, scores_ptr, stream))

    def compact_stable(self, scores_ptr: int, rows_ptr: int, ld: int, cols: int, n: int, eps: float, out_ptr: int,
                       count_ptr: int, stream: int):
        check(lib.sps_compact_stable(self.handle, scores_ptr, rows_ptr, ld, cols, n, eps, out_ptr, count_ptr, stream))

    def filter_finish(self, scores_ptr: int, n: int, raw_ptr, ld: int, cols: int, label_col: int, batch_ptr, counts_ptr,
                      eps: float, keep_strict: bool, filtered_ptr, count_ptr, labels_ptr, cloud_tr_ptr, submap_ptr, sums_ptr,
                      stream: int):
        """sps_filter_finish (include/sps_hip.h): label_col = -1 for a scan without labels; any output pointer may be None."""
        check(lib.sps_filter_finish(self.handle, scores_ptr, n, raw_ptr, ld, cols, label_col, batch_ptr, counts_ptr, eps,
                                    1 if keep_strict else 0, filtered_ptr, count_ptr, labels_ptr, cloud_tr_ptr, submap_ptr,
                                    sums_ptr, stream))

    # ---- online baseline filters (include/sps_hip.h, "online baseline filters") ----
    def transform_rows(self, xyz_ptr: int, in_f64: bool, ld: int, n: int, T, t: float, rows_ptr: int, ldo: int, feat_ptr,
                       feat_value: float, stream: int):
        check(lib.sps_transform_rows(self.handle, xyz_ptr, int(in_f64), ld, n, self._mat(T), float(t), rows_ptr, ldo, feat_ptr,
                                     float(feat_value), stream))

    def transform_points_n(self, xyz_ptr: int, in_f64: bool, ld: int, n_max: int, n_dev_ptr: int, T, out_ptr: int,
                           out_f64: bool, ldo: int, stream: int):
        check(lib.sps_transform_points_n(self.handle, xyz_ptr, int(in_f64), ld, n_max, n_dev_ptr, self._mat(T), out_ptr,
                                         int(out_f64), ldo, stream))

    def radius_crop(self, map_ptr: int, in_f64: bool, ld: int, m: int, T, r: float, scratch_ptr: int, n_scan: int,
                    rows_ptr: int, ldo: int, cap: int, feat_ptr, feat_value: float, counts_ptr: int, stream: int):
        check(lib.sps_radius_crop(self.handle, map_ptr, int(in_f64), ld, m, self._mat(T), float(r), scratch_ptr, n_scan,
                                  rows_ptr, ldo, cap, feat_ptr, float(feat_value), counts_ptr, stream))

    def label_filter(self, logits_ptr: int, ld_logits: int, n: int, rows_ptr: int, ld: int, gt_ptr, ld_gt: int,
                     labels_ptr: int, out_ptr: int, counts_ptr: int, stream: int):
        check(lib.sps_label_filter(self.handle, logits_ptr, ld_logits, n, rows_ptr, ld, gt_ptr, ld_gt, labels_ptr, out_ptr,
                                   counts_ptr, stream))

    # ---- localiser (include/sps_hip.h, "localiser") ----
    def radius_grid_upload(self, keys_ptr: int, start_ptr: int, pts_ptr: int, xyz_ptr: int, n_cells: int, m: int,
                           cell_size: float, r: float, stream: int):
        check(lib.sps_radius_grid_upload(self.handle, keys_ptr, start_ptr, pts_ptr, xyz_ptr, int(n_cells), int(m),
                                         float(cell_size), float(r), stream))

    def loc_downsample(self, rows_ptr, ld: int, n_max: int, n_dev_ptr: int, leaf: float, out_ptr, cap: int, count_ptr: int,
                       scratch_ptr: int, stream: int):
        check(lib.sps_loc_downsample(self.handle, rows_ptr, int(ld), int(n_max), n_dev_ptr, float(leaf), out_ptr, int(cap),
                                     count_ptr, scratch_ptr, stream))

    def loc_align(self, pts_ptr, n_dev_ptr: int, cap: int, T_init, iters: int, min_corr: int, tol_t: float, tol_r: float,
                  T_out_ptr: int, status_ptr: int, trace_ptr, normal_ptr, scratch_ptr: int, stream: int):
        check(lib.sps_loc_align(self.handle, pts_ptr, n_dev_ptr, int(cap), self._mat(T_init), int(iters), int(min_corr),
                                float(tol_t), float(tol_r), T_out_ptr, status_ptr, trace_ptr, normal_ptr, scratch_ptr, stream))

    # ---- localiser, scan-matching status (include/sps_hip.h, "localiser, scan-matching status") ----
    def loc_match_status(self, pts_ptr, n_dev_ptr: int, cap: int, T_dev_ptr: int, gate_in_ptr, max_distance: float,
                         max_range: float, min_inlier_fraction: float, max_error: float, min_valid: int, out_ptr: int, d2_ptr,
                         scratch_ptr: int, stream: int):
        check(lib.sps_loc_match_status(self.handle, pts_ptr, n_dev_ptr, int(cap), T_dev_ptr, gate_in_ptr, float(max_distance),
                                       float(max_range), float(min_inlier_fraction), float(max_error), int(min_valid), out_ptr,
                                       d2_ptr, scratch_ptr, stream))

    # ---- NDT localiser (include/sps_hip.h, "NDT localiser") ----
    def ndt_map_build(self, keys_ptr, start_ptr, pts_ptr, xyz_ptr, n_cells: int, n_map: int, resolution: float,
                      min_points: int, eig_ratio: float, stream: int):
        check(lib.sps_ndt_map_build(self.handle, keys_ptr, start_ptr, pts_ptr, xyz_ptr, int(n_cells), int(n_map),
                                    float(resolution), int(min_points), float(eig_ratio), stream))

    def ndt_map_cells(self, key_ptr, count_ptr, mean_ptr, icov_ptr, valid_ptr):
        self._ndt_level_call("cells", None, key_ptr, count_ptr, mean_ptr, icov_ptr, valid_ptr)

    # What is registered, the thinned points or the scan's own cells ("NDT localiser, distribution to distribution"), changes
    # the name of the ABI function and what the first three arguments hold: ``d2d`` True: the source records, n_src and
    # cap_src in the place of pts, n_dev and cap.  The ``_d2d`` methods further down are these with ``d2d=True``.
    def ndt_align(self, pts_ptr, n_dev_ptr: int, cap: int, T_init, iters: int, neighbours: int, min_corr: int,
                  outlier_ratio: float, tol_t: float, tol_r: float, T_out_ptr: int, status_ptr: int, trace_ptr, normal_ptr,
                  scratch_ptr: int, stream: int, d2d: bool = False):
        fn = lib.sps_ndt_align_d2d if d2d else lib.sps_ndt_align
        check(fn(self.handle, pts_ptr, n_dev_ptr, int(cap), self._mat(T_init), int(iters), int(neighbours), int(min_corr),
                 float(outlier_ratio), float(tol_t), float(tol_r), T_out_ptr, status_ptr, trace_ptr, normal_ptr, scratch_ptr,
                 stream))

    def ndt_align_batch(self, pts_ptr, n_dev_ptr: int, cap: int, T_init_ptr, n_hyp: int, iters: int, neighbours: int,
                        min_corr: int, outlier_ratio: float, tol_t: float, tol_r: float, T_out_ptr: int, status_ptr: int,
                        trace_ptr, normal_ptr, final_ptr: int, best_ptr: int, T_best_ptr: int, scratch_ptr: int, stream: int,
                        d2d: bool = False):
        fn = lib.sps_ndt_align_d2d_batch if d2d else lib.sps_ndt_align_batch
        check(fn(self.handle, pts_ptr, n_dev_ptr, int(cap), T_init_ptr, int(n_hyp), int(iters), int(neighbours), int(min_corr),
                 float(outlier_ratio), float(tol_t), float(tol_r), T_out_ptr, status_ptr, trace_ptr, normal_ptr, final_ptr,
                 best_ptr, T_best_ptr, scratch_ptr, stream))

    # ---- NDT localiser, pose search (include/sps_hip.h, "NDT localiser, pose search") ----
    def ndt_score_poses(self, pts_ptr, n_dev_ptr: int, cap: int, T_ptr, n_pose: int, neighbours: int, outlier_ratio: float,
                        score_ptr: int, scratch_ptr: int, stream: int, d2d: bool = False):
        fn = lib.sps_ndt_score_poses_d2d if d2d else lib.sps_ndt_score_poses
        check(fn(self.handle, pts_ptr, n_dev_ptr, int(cap), T_ptr, int(n_pose), int(neighbours), float(outlier_ratio),
                 score_ptr, scratch_ptr, stream))

    def ndt_top_poses(self, score_ptr: int, T_ptr, n_pose: int, min_corr: int, k: int, top_index_ptr: int, T_top_ptr: int,
                      n_top_ptr: int, stream: int):
        check(lib.sps_ndt_top_poses(self.handle, score_ptr, T_ptr, int(n_pose), int(min_corr), int(k), top_index_ptr, T_top_ptr,
                                    n_top_ptr, stream))

    # ---- NDT localiser, global search (include/sps_hip.h, "NDT localiser, global search") ----
    def bbs_map_build(self, g0_ptr: int, W: int, H: int, levels: int, stream: int):
        check(lib.sps_bbs_map_build(self.handle, g0_ptr, int(W), int(H), int(levels), stream))

    def bbs_map_level(self, level: int, out_ptr: int):
        """level ``level`` as stored, (H + pad) x (W + pad) bytes, into a device array; synchronises"""
        check(lib.sps_bbs_map_level(self.handle, int(level), out_ptr))

    def bbs_search(self, pts_ptr, n_dev_ptr: int, cap: int, T_up, resolution: float, i0: int, j0: int, scan_z_lo: float,
                   scan_z_hi: float, yaw_cs_ptr: int, n_yaw: int, frontier: int, min_score: int, k: int, top_index_ptr: int,
                   top_score_ptr: int, T_top_ptr: int, n_top_ptr: int, info_ptr: int, trace_ptr, scratch_ptr: int, stream: int):
        check(lib.sps_bbs_search(self.handle, pts_ptr, n_dev_ptr, int(cap), self._mat(T_up), float(resolution), int(i0), int(j0),
                                 float(scan_z_lo), float(scan_z_hi), yaw_cs_ptr, int(n_yaw), int(frontier), int(min_score), int(k),
                                 top_index_ptr, top_score_ptr, T_top_ptr, n_top_ptr, info_ptr, trace_ptr, scratch_ptr, stream))

    # ---- NDT localiser, online map (include/sps_hip.h, "NDT localiser, online map") ----
    def ndt_map_build_dynamic(self, keys_ptr, start_ptr, pts_ptr, xyz_ptr, n_cells: int, n_map: int, resolution: float,
                              min_points: int, eig_ratio: float, cell_capacity: int, stream: int):
        check(lib.sps_ndt_map_build_dynamic(self.handle, keys_ptr, start_ptr, pts_ptr, xyz_ptr, int(n_cells), int(n_map),
                                            float(resolution), int(min_points), float(eig_ratio), int(cell_capacity), stream))

    def ndt_map_update(self, *args):
        """the arguments of ``_ndt_update`` after ``pyramid``; info_ptr: int32[4]"""
        self._ndt_update(False, *args)

    def ndt_map_info(self):
        """(cells assigned, cell capacity, cells dropped for capacity since the build); synchronises"""
        return self._ndt_info(None)

    # ---- free-space carving (include/sps_hip.h, "NDT localiser, online map: free-space carving") ----
    def ndt_map_carve(self, *args):
        """the arguments of ``_ndt_carve`` after ``pyramid``; end_margin: a float; info_ptr: int32[4]"""
        self._ndt_carve(False, *args)

    def ndt_map_carve_cells(self, pass_ptr, hit_ptr, miss_ptr):
        """pass, hit and miss of every cell of the capacity into int32 device arrays (any may be None); synchronises"""
        self._ndt_level_call("carve_cells", None, pass_ptr, hit_ptr, miss_ptr)

    # The online map is a pyramid of one level (include/sps_hip.h), so its ABI functions and the online pyramid's differ by
    # their names and a level argument: one helper per pair.  ``pyramid`` False / ``level`` None: the single map.
    def _ndt_update(self, pyramid: bool, pts_ptr, n_dev_ptr: int, cap: int, T_host, T_dev_ptr, gate_ptr, max_cell_points: int,
                    info_ptr: int, scratch_ptr: int, stream: int):
        """info_ptr: int32[4], of a pyramid int32[n_levels][4]"""
        fn = lib.sps_ndt_pyramid_update if pyramid else lib.sps_ndt_map_update
        check(fn(self.handle, pts_ptr, n_dev_ptr, int(cap), self._mat(T_host) if T_host is not None else None, T_dev_ptr, gate_ptr,
                 int(max_cell_points), info_ptr, scratch_ptr, stream))

    def _ndt_carve(self, pyramid: bool, pts_ptr, n_dev_ptr: int, cap: int, T_host, T_dev_ptr, gate_ptr, end_margin,
                   through_sigma: float, min_pass: int, miss_frames: int, max_steps: int, info_ptr: int, scratch_ptr, stream: int):
        """end_margin: a float, of a pyramid one float per level; info_ptr: as for ``_ndt_update``"""
        fn = lib.sps_ndt_pyramid_carve if pyramid else lib.sps_ndt_map_carve
        em = (C.c_double * len(end_margin))(*[float(v) for v in end_margin]) if pyramid else float(end_margin)
        check(fn(self.handle, pts_ptr, n_dev_ptr, int(cap), self._mat(T_host) if T_host is not None else None, T_dev_ptr, gate_ptr,
                 em, float(through_sigma), int(min_pass), int(miss_frames), int(max_steps), info_ptr, scratch_ptr, stream))

    def _ndt_level_call(self, name: str, level, *args):
        """sps_ndt_map_<name>(ctx, args) or, with a level, sps_ndt_pyramid_<name>(ctx, level, args); name: info, cells or
        carve_cells"""
        if level is None:
            check(getattr(lib, f"sps_ndt_map_{name}")(self.handle, *args))
        else:
            check(getattr(lib, f"sps_ndt_pyramid_{name}")(self.handle, int(level), *args))

    def _ndt_info(self, level):
        out = (C.c_int64 * 4)()
        self._ndt_level_call("info", level, out)
        return int(out[0]), int(out[1]), int(out[2])

    # ---- NDT localiser, multi-resolution pyramid (include/sps_hip.h, "NDT localiser, multi-resolution pyramid") ----
    def ndt_pyramid_build(self, levels, xyz_ptr, n_map: int, min_points: int, eig_ratio: float, outlier_ratio: float,
                          stream: int, cell_capacity=None):
        """levels: per level, coarsest first, (keys_ptr, start_ptr, pts_ptr, n_cells, resolution); cell_capacity (one int
        per level): the dynamic pyramid of the "NDT localiser, online pyramid" section"""
        L = len(levels)
        keys, start, pts = ((C.c_void_p * L)(*[lv[i] for lv in levels]) for i in range(3))
        n_cells = (C.c_int64 * L)(*[int(lv[3]) for lv in levels])
        res = (C.c_double * L)(*[float(lv[4]) for lv in levels])
        if cell_capacity is None:
            check(lib.sps_ndt_pyramid_build(self.handle, L, keys, start, pts, n_cells, res, xyz_ptr, int(n_map), int(min_points),
                                            float(eig_ratio), float(outlier_ratio), stream))
            return
        if len(cell_capacity) != L:
            raise ValueError("cell_capacity needs one entry per level")
        caps = (C.c_int64 * L)(*[int(v) for v in cell_capacity])
        check(lib.sps_ndt_pyramid_build_dynamic(self.handle, L, keys, start, pts, n_cells, res, xyz_ptr, int(n_map),
                                                int(min_points), float(eig_ratio), float(outlier_ratio), caps, stream))

    # ---- NDT localiser, online pyramid (include/sps_hip.h, "NDT localiser, online pyramid") ----
    def ndt_pyramid_update(self, *args):
        """the arguments of ``_ndt_update`` after ``pyramid``; info_ptr: int32[n_levels][4]"""
        self._ndt_update(True, *args)

    def ndt_pyramid_carve(self, *args):
        """the arguments of ``_ndt_carve`` after ``pyramid``; end_margin: one float per level; info_ptr: int32[n_levels][4]"""
        self._ndt_carve(True, *args)

    def ndt_pyramid_info(self, level: int):
        """(cells assigned, cell capacity, cells dropped for capacity since the build) of a level; synchronises"""
        return self._ndt_info(level)

    def ndt_pyramid_carve_cells(self, level: int, pass_ptr, hit_ptr, miss_ptr):
        """pass, hit and miss of every cell of a level's capacity into int32 device arrays (any may be None); synchronises"""
        self._ndt_level_call("carve_cells", level, pass_ptr, hit_ptr, miss_ptr)

    def ndt_pyramid_cells(self, level: int, key_ptr, count_ptr, mean_ptr, icov_ptr, valid_ptr):
        self._ndt_level_call("cells", level, key_ptr, count_ptr, mean_ptr, icov_ptr, valid_ptr)

    def ndt_pyramid_align(self, pts_ptr, n_dev_ptr: int, cap: int, T_init, iters: int, level_iters, neighbours: int,
                          min_corr: int, tol_t: float, tol_r: float, T_out_ptr: int, status_ptr: int, trace_ptr, normal_ptr,
                          level_ptr, scratch_ptr: int, stream: int, d2d: bool = False):
        """d2d: src [L][cap][NDT_SRC_REC] and n_src [L][2] for pts and n_dev, as ``ndt_pyramid_source_build`` leaves them"""
        fn = lib.sps_ndt_pyramid_align_d2d if d2d else lib.sps_ndt_pyramid_align
        caps = (C.c_int32 * len(level_iters))(*[int(v) for v in level_iters])
        check(fn(self.handle, pts_ptr, n_dev_ptr, int(cap), self._mat(T_init), int(iters), caps, int(neighbours),
                 int(min_corr), float(tol_t), float(tol_r), T_out_ptr, status_ptr, trace_ptr, normal_ptr, level_ptr,
                 scratch_ptr, stream))

    # ---- NDT localiser, pyramid, several hypotheses (include/sps_hip.h, same title) ----
    def ndt_pyramid_align_batch(self, pts_ptr, n_dev_ptr: int, cap: int, T_init_ptr, n_hyp: int, iters: int, level_iters,
                                neighbours: int, min_corr: int, tol_t: float, tol_r: float, T_out_ptr: int, status_ptr: int,
                                trace_ptr, normal_ptr, level_ptr, final_ptr: int, best_ptr: int, T_best_ptr: int,
                                scratch_ptr: int, stream: int, d2d: bool = False):
        """d2d: src [L][cap][NDT_SRC_REC] and n_src [L][2] for pts and n_dev, as ``ndt_pyramid_source_build`` leaves them"""
        fn = lib.sps_ndt_pyramid_align_d2d_batch if d2d else lib.sps_ndt_pyramid_align_batch
        caps = (C.c_int32 * len(level_iters))(*[int(v) for v in level_iters])
        check(fn(self.handle, pts_ptr, n_dev_ptr, int(cap), T_init_ptr, int(n_hyp), int(iters), caps,
                 int(neighbours), int(min_corr), float(tol_t), float(tol_r), T_out_ptr, status_ptr, trace_ptr, normal_ptr,
                 level_ptr, final_ptr, best_ptr, T_best_ptr, scratch_ptr, stream))

    # ---- NDT localiser, distribution to distribution (include/sps_hip.h, same title) ----
    def ndt_source_build(self, pts_ptr, n_dev_ptr: int, cap: int, source_resolution: float, min_points: int, eig_ratio: float,
                         src_ptr, src_count_ptr, n_src_ptr: int, scratch_ptr: int, stream: int):
        check(lib.sps_ndt_source_build(self.handle, pts_ptr, n_dev_ptr, int(cap), float(source_resolution), int(min_points),
                                       float(eig_ratio), src_ptr, src_count_ptr, n_src_ptr, scratch_ptr, stream))

    def ndt_align_d2d(self, *args):
        """``ndt_align`` with the source records, n_src and cap_src"""
        self.ndt_align(*args, d2d=True)

    # ---- NDT localiser, distribution to distribution, several poses (include/sps_hip.h, same title) ----
    def ndt_align_d2d_batch(self, *args):
        self.ndt_align_batch(*args, d2d=True)

    def ndt_score_poses_d2d(self, *args):
        self.ndt_score_poses(*args, d2d=True)

    # ---- NDT localiser, distribution to distribution, pyramid (include/sps_hip.h, same title) ----
    def ndt_pyramid_source_build(self, pts_ptr, n_dev_ptr: int, cap: int, source_resolutions, min_points, eig_ratio: float,
                                 src_ptr, src_count_ptr, n_src_ptr: int, scratch_ptr: int, stream: int):
        """source_resolutions, min_points: one entry per level; src [L][cap][NDT_SRC_REC], src_count [L][cap], n_src [L][2]"""
        L = len(source_resolutions)
        if len(min_points) != L:
            raise ValueError("min_points needs one entry per level")
        res = (C.c_double * L)(*[float(v) for v in source_resolutions])
        mp = (C.c_int32 * L)(*[int(v) for v in min_points])
        check(lib.sps_ndt_pyramid_source_build(self.handle, pts_ptr, n_dev_ptr, int(cap), L, res, mp, float(eig_ratio), src_ptr,
                                               src_count_ptr, n_src_ptr, scratch_ptr, stream))

    def ndt_pyramid_align_d2d(self, *args):
        self.ndt_pyramid_align(*args, d2d=True)

    # ---- NDT localiser, distribution to distribution, pyramid, several hypotheses (include/sps_hip.h, same title) ----
    def ndt_pyramid_align_d2d_batch(self, *args):
        """``ndt_pyramid_align_batch`` with the levels' source records, n_src and cap_src"""
        self.ndt_pyramid_align_batch(*args, d2d=True)

    def train_forward(self, params_ptr: int, numel: int, coords_ptr: int, ld: int, n: int, voxel_size: float,
                      scores_ptr: int, batch_stats_ptr, stream: int):
        check(lib.sps_train_forward(self.handle, params_ptr, numel, coords_ptr, ld, n, voxel_size, scores_ptr,
                                    batch_stats_ptr, stream))

    def train_backward(self, dscores_ptr: int, scores_ptr: int, grad_ptr: int, numel: int, stream: int, generation=None):
        """``generation`` (train_generation() right after the forward): refuse to differentiate a forward whose activations
        a later forward on this context has overwritten."""
        if generation is None:
            check(lib.sps_train_backward(self.handle, dscores_ptr, scores_ptr, grad_ptr, numel, stream))
        else:
            check(lib.sps_train_backward_at(self.handle, int(generation), dscores_ptr, scores_ptr, grad_ptr, numel, stream))

    def train_generation(self) -> int:
        g = C.c_int64()
        check(lib.sps_train_generation(self.handle, C.byref(g)))
        return g.value

    def train_wgrad_plan(self, conv_name: str):
        """(gshift, nwg) of the weight-gradient launch of a convolution at this context's capacity (after a training forward)"""
        g, n = C.c_int32(), C.c_int32()
        check(lib.sps_train_wgrad_plan(self.handle, conv_name.encode(), C.byref(g), C.byref(n)))
        return g.value, n.value

    def level_counts(self):
        out = (C.c_int64 * NUM_LEVELS)()
        check(lib.sps_level_counts(self.handle, out))
        return list(out)

    def block_slots(self, level: int):
        """(slots of the level's block hash, int32 numpy [blocks]: the slot each block of the last forward held, by block
        rank) -- a debug view for the tests of the hash walk (include/sps_hip.h: sps_get_block_slots)"""
        import numpy as np
        ns, nb = C.c_int64(), C.c_int64()
        check(lib.sps_get_block_slots(self.handle, level, C.byref(ns), C.byref(nb), None, 0))
        out = np.zeros(nb.value, np.int32)
        if nb.value:
            check(lib.sps_get_block_slots(self.handle, level, C.byref(ns), C.byref(nb), out.ctypes.data, len(out)))
        return ns.value, out

    def kernel_map(self, which: int, source: int = 0):
        """Dense int32 [K, V_out] table of a kernel map of the last forward (include/sps_hip.h: sps_get_kernel_map), on the
        device; with source = 1 also the number of pairs the rulebook holds."""
        import torch
        counts = self.level_counts()
        level = which if which <= 4 else (0 if which == 5 else which - 5)
        K = 81 if which <= 4 else (125 if which == 5 else 8)
        out = torch.empty((K, counts[level]), dtype=torch.int32, device=f"cuda:{self.device}")
        n = C.c_int64()
        check(lib.sps_get_kernel_map(self.handle, which, source, out.data_ptr(), C.byref(n)))
        return (out, n.value) if source == 1 else out

    def rulebook_chunks(self, which: int):
        """int32 numpy [supertiles, 3]: 16-slot chunks of the level's rulebook per 64-row supertile and time slice."""
        import numpy as np
        n = C.c_int64()
        check(lib.sps_get_rulebook_chunks(self.handle, which, None, C.byref(n)))
        out = np.zeros((n.value, 3), np.int32)
        if n.value:
            check(lib.sps_get_rulebook_chunks(self.handle, which, out.ctypes.data, C.byref(n)))
        return out

    LAUNCH_FAMILIES = ("none", "k_conv", "k_conv_px", "k_upconv", "conv0")

    def conv_launch(self, conv_name: str) -> dict:
        """What the last forward launched for a layer of the wiring table (include/sps_hip.h: sps_get_conv_launch)."""
        out = (C.c_int32 * 8)()
        check(lib.sps_get_conv_launch(self.handle, conv_name.encode(), out))
        return {"family": self.LAUNCH_FAMILIES[out[0]], "ntw": out[1], "S": out[2], "U4": bool(out[3]), "fused_up": bool(out[4]),
                "order_ways": out[5], "cap": out[6], "pipelined": bool(out[7])}

    def map_pairs(self, which: int):
        out = (C.c_int64 * 125)()
        check(lib.sps_get_map_pairs(self.handle, which, out))
        return list(out)[: 125 if which == 5 else 81]


# ---- LTS baseline (include/sps_hip.h, "LTS baseline") ----------------------------------------------------------------
LTS_LIDARS = {"vlp-16": 0, "hdl-32": 1}
_LTS_LAYOUT = None


def lts_layout():
    """((name, offset, numel, shape), ...) of the LTS weight blob: the reference SPCTReg state_dict, in its order."""
    global _LTS_LAYOUT
    if _LTS_LAYOUT is None:
        out = []
        buf = C.create_string_buffer(128)
        off, num, nd = C.c_int64(), C.c_int64(), C.c_int()
        shape = (C.c_int64 * 3)()
        for i in range(lib.sps_lts_num_tensors()):
            check(lib.sps_lts_tensor_info(i, buf, 128, C.byref(off), C.byref(num), shape, C.byref(nd)))
            out.append((buf.value.decode(), off.value, num.value, tuple(shape[d] for d in range(nd.value))))
        _LTS_LAYOUT = tuple(out)
    return _LTS_LAYOUT


def lts_lidar_info(lidar: str):
    """(beams, window_size, num_windows) of a lidar name."""
    if lidar not in LTS_LIDARS:
        raise ValueError(f"unknown lidar {lidar!r}")
    b, w, nw = C.c_int(), C.c_int(), C.c_int()
    check(lib.sps_lts_lidar_info(LTS_LIDARS[lidar], C.byref(b), C.byref(w), C.byref(nw)))
    return b.value, w.value, nw.value


def lts_check(rc: int) -> None:
    """check() for the LTS calls: an out-of-image or NaN point is the reference's IndexError."""
    if rc == ERR_RANGE:
        raise IndexError(lib.sps_last_error().decode())
    check(rc)


class LtsHandle:
    """One ``sps_lts``: folded SPCTReg weights + workspace on one device."""

    def __init__(self, device: int, blob_host_ptr: int, numel: int):
        h = C.c_void_p()
        check(lib.sps_lts_create(int(device), blob_host_ptr, int(numel), C.byref(h)))
        self.handle = h
        self.device = int(device)

    def project(self, pts_ptr, ld, n, lidar: int, frame_ptr, x_ptr, rows_ptr, stream):
        check(lib.sps_lts_project(self.handle, pts_ptr, ld, n, lidar, frame_ptr, x_ptr, rows_ptr, stream))

    def forward(self, x_ptr, B, N, scores_ptr, stream):
        check(lib.sps_lts_forward(self.handle, x_ptr, B, N, scores_ptr, stream))

    def check_errors(self, stream):
        lts_check(lib.sps_lts_check(self.handle, stream))

    def tap_shape(self, which: int):
        r, c = C.c_int64(), C.c_int64()
        check(lib.sps_lts_tap(self.handle, which, None, C.byref(r), C.byref(c), None))
        return r.value, c.value

    def tap(self, which: int, out_ptr, stream):
        check(lib.sps_lts_tap(self.handle, which, out_ptr, None, None, stream))

    def close(self):
        if getattr(self, "handle", None):
            lib.sps_lts_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
