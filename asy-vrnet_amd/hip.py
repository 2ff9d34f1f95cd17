"""ctypes binding of the C-ABI in include/vrnet_hip.h (libvrnet_hip.so, gfx950).

PyTorch is used for device memory and streams only: every function below passes raw device
pointers, sizes and the current HIP stream to the library.  There is no fallback: a missing
library raises at import of this module, a failing call raises RuntimeError with the
library's message (mirroring the reference's assert at backbone/fusion/vr_coc.py:163-164).
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VRNET_HIP_LIB") or os.path.join(_HERE, "csrc", "libvrnet_hip.so")   # override: diagnostic builds only
ABI_VERSION = 11

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
        "or make -C asy-vrnet_amd/csrc). The hot path has no CPU/eager fallback.")
_lib = ctypes.CDLL(LIB_PATH)

P, L, I, F, D = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_double
_SIGS = {
    "vrnet_abi_version": ([], I),
    "vrnet_last_error": ([], ctypes.c_char_p),
    "vrnet_last_kernel": ([], I),
    "vrnet_tuning_build": ([], I),
    "vrnet_kernel_launches": ([I], L),
    "vrnet_device_arch": ([ctypes.c_char_p, I], I),
    "vrnet_conv2d_f32": ([P, L, P, P, P, L] + [I] * 14 + [P, L, P, L, P, P, P, L, I, I, I, I, P, I, I, P, P, P, P, P, P, P, L, P], I),
    "vrnet_conv2d_dma_plan": ([L, I, L, P], I),
    "vrnet_conv2d_splitk_workspace": ([L, I, L], L),
    "vrnet_conv_planes_bytes": ([I, I], L),
    "vrnet_conv_planes_pack_f32": ([P, I, L, P], I),
    "vrnet_pack_weight_t_f32": ([P, P, P, I, I, I, I, P], I),
    "vrnet_gemm_planes_ok": ([L, I, I], I),
    "vrnet_gemm_planes_f32": ([P, L, L, P, L, L, I, L, I, I, P, P, L, P, L, L, I, I, P, L, P, L, P, P, L, I, P, L, P, I, P], I),
    "vrnet_planes_split_blocks": ([L, L], L),
    "vrnet_planes_split_f32": ([P, I, L, I, P], I),
    "vrnet_planes_from_f32": ([P, L, L, L, P, L, L, I, P], I),
    "vrnet_wgrad_planes_ok": ([L, I, I], I),
    "vrnet_wgrad_planes_workspace": ([L, I, I], L),
    "vrnet_wgrad_planes_plan": ([L, I, I, I, P, P, P, P], I),
    "vrnet_wgrad_planes_f32": ([P, L, L, P, L, L, I, L, I, I, P, P, P, I, P, P, P, P, L, P], I),
    "vrnet_conv2d_dma_tile": ([L, I], I),
    "vrnet_conv2d_wgrad_workspace": ([I] * 8, L),
    "vrnet_conv2d_wgrad_plan": ([L] + [I] * 8 + [P], I),
    "vrnet_conv2d_plan": ([I] * 14 + [L, L, I, L, P], I),
    "vrnet_conv2d_wgrad_f32": ([P, L, P, L, P, P, P] + [I] * 14 + [P, P, P, P, P, P, P, P, P, P, L, P], I),
    "vrnet_pack_weight_f32": ([P, P, I, I, I, I, P], I),
    "vrnet_mlp_fused_ok": ([I, I, L], I),
    "vrnet_mlp_rc_ok": ([I, I, L], I),
    "vrnet_mlp_pack_bytes": ([I, I, I], L),
    "vrnet_mlp_pack_f32": ([P, P, I, I, I, P, P, P], I),
    "vrnet_mlp_fwd_f32": ([P, L, P, P, P, P, L, P, P, L, P, L, P, L, I, I, I, P], I),
    "vrnet_mlp_pack_rc_bytes": ([I, I, I], L),
    "vrnet_mlp_pack_rc_f32": ([P, P, I, I, I, P, P], I),
    "vrnet_mlp_bwd_rc_f32": ([P, L, P, P, P, L, P, P, L, P, L, P, L, L, I, I, I, P], I),
    "vrnet_mlp_bwd_f32": ([P, L, P, P, P, L, P, L, P, L, P, L, L, I, I, I, P], I),
    "vrnet_moments_workspace": ([I, L, I], L),
    "vrnet_moments_f32": ([P, L, P, L, P, L, I, L, I, P, P, L, P], I),
    "vrnet_affine_f32": ([P, L, P, P, P, I, P, L, P, L, P, P, P, L, P, L, I, L, I, I, P, L, P], I),
    "vrnet_gn_coef_fwd": ([P, P, P, F, I, L, I, P, P, P, P, P], I),
    "vrnet_gn_coef_from_pairs": ([P, L, P, P, F, I, L, I, P, P, P, P, P, P, P], I),
    "vrnet_gn_stats_fwd": ([P, L, P, P, F, I, L, I, P, P, P, P, P, P, P, L, P], I),
    "vrnet_gn_coef_bwd": ([P, P, P, I, L, I, P, P, P, P, P, P, I, P, P, P, P], I),
    "vrnet_gn_apply_fwd": ([P, L, P, L, P, P, F, I, L, I, P, L, P, P], I),
    "vrnet_gn_apply_fwd_planes": ([P, L, P, L, P, P, F, I, L, I, P, L, P, P, P], I),
    "vrnet_gn_apply_bwd_planes": ([P, L, P, L, P, P, I, L, I, P, L, P, L, P, P, I, P, P, L, P], I),
    "vrnet_cluster_fwd_planes_f32": ([P, P, L, I, P, P, P, L, P, P, I, I, I, I, I, I, I, P, P, P], I),
    "vrnet_cluster_state_floats": ([I, I, I, I, I], L),
    "vrnet_cluster_bwd_planes_f32": ([P, P, L, I, P, P, P, P, L, P, P, L, P, P, I, I, I, I, I, I, I, P, P, P, P, L, P], I),
    "vrnet_gn_bwd_workspace": ([I, L, I], L),
    "vrnet_gn_apply_bwd_from_partials": ([P, L, P, L, P, P, P, P, I, L, I, P, L, P, L, P, P, I, P], I),
    "vrnet_bn_coef_fwd_from_partials": ([P, P, P, F, F, P, P, P, I, L, I, P, P, P, P, P], I),
    "vrnet_gn_apply_bwd": ([P, L, P, L, P, P, I, L, I, P, L, P, L, P, P, I, P, L, P], I),
    "vrnet_bn_coef_fwd": ([P, P, P, F, F, P, P, P, I, I, L, I, P, P, P, P, P], I),
    "vrnet_bn_coef_bwd": ([P, P, P, I, I, L, I, P, P, P, P, P, P, I, P], I),
    "vrnet_bn_stats_fwd": ([P, L, P, P, F, F, P, P, P, I, L, I, P, P, P, P, P, L, P], I),
    "vrnet_bn_stats_bwd_zmask": ([P, L, P, L, P, P, P, P, P, I, I, L, I, P, P, P, P, P, P, I, P, L, P], I),
    "vrnet_bn_apply_bwd_zmask": ([P, L, P, L, P, P, P, P, P, P, P, P, L, I, L, I, P], I),
    "vrnet_bn_stats_bwd": ([P, L, P, L, P, L, P, P, I, I, L, I, P, P, P, P, P, P, I, P, L, P], I),
    "vrnet_eca_coef_fwd": ([P, P, I, I, L, I, P, P], I),
    "vrnet_eca_coef_bwd": ([P, P, P, P, I, I, L, I, P, P, I, P], I),
    "vrnet_ls_coef_bwd": ([P, P, I, I, P, P, I, I, P, P, P, P], I),
    "vrnet_moments_to_float": ([P, P, L, D, I, P], I),
    "vrnet_copy_channels_f32": ([P, L, I, P, L, I, L, I, I, P], I),
    "vrnet_cat2_f32": ([P, L, I, P, L, I, P, L, L, I, I, I, I, P], I),
    "vrnet_patch_gather_f32": ([P, L, P, P, I, I, I, I, I, I, P], I),
    "vrnet_patch_scatter_f32": ([P, P, L, I, I, I, I, I, I, I, P], I),
    "vrnet_weight_ohwi_f32": ([P, P, I, I, I, I, I, I, P], I),
    "vrnet_nchw_to_nhwc_f32": ([P, P, L, I, I, L, P], I),
    "vrnet_nhwc_to_nchw_f32": ([P, L, P, I, I, L, I, P], I),
    "vrnet_add_f32": ([P, P, L, P], I),
    "vrnet_fill_f32": ([P, F, L, P], I),
    "vrnet_cluster_fwd_f32": ([P, P, L, P, P, P, L, P, P, I, I, I, I, I, I, P, P, P], I),
    "vrnet_cluster_fwd_forced_f32": ([P, P, L, P, P, P, L, P, P, I, I, I, I, I, I, P, P, P], I),
    "vrnet_cluster_plan": ([I, L, I, P, P], I),
    "vrnet_cluster_bwd_workspace": ([I, I, I], L),
    "vrnet_cluster_bwd_workspace2": ([I, I, I, I, I], L),
    "vrnet_cluster_bwd_f32": ([P, P, L, P, P, P, P, L, P, P, L, P, P, I, I, I, I, I, I, I, P, P, P, P, P, L, P], I),
    "vrnet_cluster_ab_reduce_multi": ([I, P, P, P, P, P, P], I),
    "vrnet_dwconv3x3_f32": ([P, L, P, P, L, I, I, I, I, I, I, P], I),
    "vrnet_dwconv3x3_wgrad_workspace": ([I, I, I, I], L),
    "vrnet_dwconv3x3_wgrad_f32": ([P, L, P, L, P, I, I, I, I, I, P, L, P], I),
    "vrnet_upsample_bilinear_f32": ([P, L, P, L, I, I, I, I, I, I, P], I),
    "vrnet_bn_relu_upsample_bilinear_f32": ([P, L, P, P, P, P, L, I, I, I, I, I, I, P], I),
    "vrnet_upsample_bilinear_bwd_f32": ([P, L, I, P, L, I, I, I, I, I, I, P], I),
    "vrnet_up_cat_ok": ([I, I, L, L, L, I], I),
    "vrnet_up_cat_pairs": ([I, L, I], L),
    "vrnet_bn_relu_upsample_cat_f32": ([P, L, P, P, P, P, L, P, L, I, I, I, I, I, I, I, I, I, P, P, L, P], I),
    "vrnet_upsample_bilinear_bwd_cat_f32": ([P, L, I, I, P, L, I, I, I, I, I, I, P], I),
    "vrnet_reduce_workspace": ([], L),
    "vrnet_minmax_f32": ([P, L, P, P, L, P], I),
    "vrnet_enhance_mul_f32": ([P, P, P, P, L, P], I),
    "vrnet_enhance_fwd_f32": ([P, P, P, P, L, P, L, P], I),
    "vrnet_fusion_chunks": ([L, I], I),
    "vrnet_fusion_fold_chunks": ([L, I], I),
    "vrnet_bn_relu_minmax_f32": ([P, P, P, P, P, L, I, P, P], I),
    "vrnet_bn_relu_res_stats_f32": ([P, P, P, P, P, P, L, I, P, P], I),
    "vrnet_enhance_stats_f32": ([P, P, P, I, P, P, L, I, P, P], I),
    "vrnet_bn_bwd_enhance_f32": ([P, P, P, P, P, P, P, P, P, P, L, I, P, P], I),
    "vrnet_enhance_bwd_stats_f32": ([P, P, P, P, P, I, P, P, P, P, P, P, L, I, I, P, P], I),
    "vrnet_bn_bwd_next_stats_f32": ([P, P, P, P, P, P, P, P, P, P, P, L, I, P, P], I),
    "vrnet_bn_coef_fwd_from_chunks": ([P, I, L, P, P, F, F, P, P, P, I, P, P, P, P, P], I),
    "vrnet_bn_coef_bwd_from_chunks": ([P, I, L, P, P, I, I, P, P, P, P, P, P, I, P], I),
    "vrnet_enhance_bwd_f32": ([P, P, P, P, P, P, L, I, P, L, P], I),
    "vrnet_sa_coef_fwd": ([P] * 7 + [I, L, I, I, P, P, P, P], I),
    "vrnet_sa_cat_sums_f32": ([P, L, P, P, P, P, L, P, L, I, L, I, P, P, L, P], I),
    "vrnet_sa_apply_f32": ([P, L, P, P, P, P, L, I, L, I, P], I),
    "vrnet_sa_bwd_workspace": ([I, L, I], L),
    "vrnet_decode_outputs_f32": ([P, P, P, I, I, I, F, F, P, P], I),
    "vrnet_detect_select_f32": ([P, I, I, I, I, F, P, P, P, P, P, P], I),
    "vrnet_nms_workspace_bytes": ([I, I], L),
    "vrnet_nms_segmented_f32": ([P, I, P, P, P, P, I, L, I, D, P, L, P, P, P, P], I),
    "vrnet_nms_capped_f32": ([P, I, P, P, P, P, I, L, I, D, P, L, P, P, P, P, P], I),
    "vrnet_detect_finish_f32": ([P, P, I, I, I, I, I, D, D, D, D, P, P, P, P, P, P], I),
    "vrnet_eval_append_f32": ([P, P, I, I, P, P, I, P, I, I, P, P, P, P, P, P, P, P, P], I),
    "vrnet_batch_formats_u8":([P, P, I, I, I, I, P, P, P, P], I),
    "vrnet_radar_workspace_bytes": ([I], L),
    "vrnet_radar_normalise": ([P, I, I, L, I, P, P, L, P], I),
    "vrnet_letterbox_workspace": ([I, I, I, I, I], L),
    "vrnet_letterbox_u8": ([P, P] + [I] * 9 + [P, P, P, P, L, P], I),
    "vrnet_render_u8": ([P, P, I, I, I, P, I, I, F, P, P, I, P, I, I, P, P, P, P], I),
    "vrnet_letterbox_ragged_workspace": ([I] * 6, L),
    "vrnet_letterbox_ragged_u8": ([P, P, P] + [I] * 6 + [P, P, P, P, P, L, P], I),
    "vrnet_detect_finish_ragged_f32": ([P, P, P, I, I, I, I, I, P, P, P, P, P, P], I),
    "vrnet_seg_predict_ragged_workspace": ([I, I, I, I], L),
    "vrnet_seg_predict_ragged_f32": ([P, P, I, I, I, I, I, I, P, P, P, L, P], I),
    "vrnet_render_ragged_u8": ([P, P, P, I, I, I, P, I, I, F, P, P, I, P, I, P, P, P, P], I),
    "vrnet_seg_targets_ragged_u8": ([P, P, I, I, I, I, I, I, P, P, P, P], I),
    "vrnet_box_targets_ragged_f32": ([P, P, P, I, I, I, I, I, I, P, P, P, P], I),
    "vrnet_augment_frames_u8": ([P, P] + [I] * 6 + [P, P, P, P, L, P], I),
    "vrnet_augment_seg_targets_u8": ([P, P, I, I, I, I, I, I, P, P, P, P], I),
    "vrnet_augment_box_targets_f32": ([P, P, P, I, I, I, I, I, I, P, P, P, P], I),
    "vrnet_augment_radar_f32": ([P, P, I, I, I, I, I, P, P, P], I),
    "vrnet_augment_post_frames_u8": ([P, P, P] + [I] * 6 + [P, P, P, P], I),
    "vrnet_augment_post_seg_targets_i64": ([P, P, I, I, I, I, I, P, P, P, P], I),
    "vrnet_augment_post_box_targets_f32": ([P, P, P, P] + [I] * 7 + [P, P, P, P], I),
    "vrnet_augment_post_radar_f32": ([P, P, I, I, I, I, P, P, P], I),
    "vrnet_mosaic_workspace_bytes": ([I] * 6, L),
    "vrnet_mosaic_frames_u8": ([P, I, P] + [I] * 6 + [P, P, P, P, L, P], I),
    "vrnet_mosaic_seg_targets_u8": ([P, I, P, I, I, I, I, I, I, P, P, P, P], I),
    "vrnet_mosaic_box_targets_f32": ([P, P, I, P, I, I, I, I, I, I, P, P, P, P], I),
    "vrnet_mosaic_radar_f32": ([P, I, P, I, I, I, I, I, P, P, P], I),
    "vrnet_radar_map_workspace": ([I, I, I], L),
    "vrnet_radar_map_f32": ([P, I, P, I, I, I, I, F, P, P, P, L, P], I),
    "vrnet_radar_map_post_f32": ([P, I, P, I, I, I, I, F, P, I, P, P, P, L, P], I),
    "vrnet_box_radar_workspace": ([I, I], L),
    "vrnet_box_radar_f32": ([P, I, P, I, P, P, I, F, F, P, P, P, P, L, P], I),
    "vrnet_track_update_f32": ([P, P, I, I, P, I, P, P, P, P, F, I, F, F, F, F, P, P], I),
    "vrnet_seg_regions_workspace_bytes": ([I, I, I], L),
    "vrnet_seg_regions_u8": ([P, I, I, I, P, I, I, P, P, I, I, I, I, I, I, P, I, P, P, P, P, P, P, L, P], I),
    "vrnet_mosaic_radar_points_workspace": ([I, I, I], L),
    "vrnet_mosaic_radar_points_f32": ([P, I, I, P, P, I, I, I, I, I, I, F, P, P, P, L, P], I),
    "vrnet_label_index_f32": ([P, P, P, I, I, I, P, I, P, P], I),
    "vrnet_render_labels_u8": ([P, I, I, I, P, P, I, P, I, I, P, P, L, P, I, I, I, P, P], I),
    "vrnet_render_labels_ragged_u8": ([P, P, P, I, I, I, P, P, I, P, I, P, P, L, P, I, I, P, P], I),
    "vrnet_caption_text_f32": ([P, P, P, I, I, P, I, P, P, F, P, I, P, P], I),
    "vrnet_render_captions_u8": ([P, I, I, I, P, P, I, P, I, P, P, L, P, I, I, P, P], I),
    "vrnet_render_captions_ragged_u8": ([P, P, P, I, I, I, P, P, I, P, I, P, P, L, P, I, P, P], I),
    "vrnet_crop_boxes_u8": ([P, I, I, I, P, P, P, I, P, L, P, P, P, P], I),
    "vrnet_chip_workspace": ([I, I, I], L),
    "vrnet_chip_boxes_u8": ([P, I, I, I, P, P, P, I, I, I, I, P, P, P, P, P, P, P], I),
    "vrnet_jpeg_workspace_bytes": ([I, I, I, I, L], L),
    "vrnet_jpeg_encode_u8": ([P, I, I, I, P, P, I, P, P, L, P, P, P, L, P], I),
    "vrnet_dehaze_workspace_bytes": ([I, I, I], L),
    "vrnet_dehaze_u8": ([P, P, I, I, I, I, I, D, D, D, P, P, P, P, L, P], I),
    "vrnet_ace_workspace_bytes": ([I, I, I], L),
    "vrnet_ace_u8": ([P, P, I, I, I, I, D, D, I, P, P, P, P, L, P], I),
    "vrnet_heatmap_workspace": ([I, I, I], L),
    "vrnet_heatmap_f32": ([P, P, P] + [I] * 11 + [P, P, F, P, P, P, P, L, P], I),
    "vrnet_heatmap_ragged_workspace": ([I, I, I], L),
    "vrnet_heatmap_ragged_f32": ([P, P, P, P] + [I] * 7 + [P, P, F, P, P, P, P, P, L, P], I),
    "vrnet_yolo_loss_workspace": ([I, L, I, I], L),
    "vrnet_yolo_loss_f32": ([P, P, P, P, P, I, I, I, P, P, I, F, P, P, P, P, P, L, P], I),
    "vrnet_seg_loss_workspace": ([I, I, L], L),
    "vrnet_seg_loss_f32": ([P, P, P, P, I, I, L, I, I, F, F, F, F, F, P, P, P, L, P], I),
    "vrnet_seg_fscore_f32": ([P, P, I, I, L, F, F, F, P, P, P, L, P], I),
    "vrnet_seg_predict_workspace": ([I, I, I, I], L),
    "vrnet_seg_predict_f32": ([P, I, I, I, I, I, I, I, I, I, I, P, P, L, P], I),
    "vrnet_confusion_hist": ([P, I, P, I, L, I, P, P], I),
    "vrnet_det_map_workspace_bytes": ([I, I, I], L),
    "vrnet_det_map_f64": ([P, P, P, P, P, P, I, P, P, P, P, I, I, I, P, I, D] + [P] * 15 + [P, L, P], I),
    "vrnet_coco_map_group_bytes": ([I, I], L),
    "vrnet_coco_map_workspace_bytes": ([I, L], L),
    "vrnet_coco_map_f64": ([P, P, P, P, P, I, P, P, P, I, I, L, P, P, P, P, P, I, I, I] + [P] * 9 + [L, P], I),
    "vrnet_mean_square_workspace": ([I, P], L),
    "vrnet_mean_square_f32": ([I, P, P, P, P, L, P], I),
    "vrnet_mean_square_bwd_f32": ([I, P, P, P, P, P], I),
    "vrnet_mt_sgd_f32": ([P, P, P, P, P, I, I, I, F, F, I, I, P], I),
    "vrnet_mt_adam_f32": ([P, P, P, P, P, I, I, I, F, F, F, F, I, P], I),
    "vrnet_mt_ema_f32": ([P, P, P, P, I, I, I, F, P], I),
    "vrnet_mt_sgd_dev_f32": ([P, P, P, P, P, I, I, I, P, F, I, P], I),
    "vrnet_mt_adam_dev_f32": ([P, P, P, P, P, I, I, I, P, F, F, F, P], I),
    "vrnet_mt_ema_dev_f32": ([P, P, P, P, I, I, I, P, P], I),
    "vrnet_adam_bias_correction": ([F, F, I, ctypes.POINTER(F), ctypes.POINTER(F)], I),
    "vrnet_clock_stamp": ([P, P], I),
    "vrnet_mt_copy_f32": ([P, P, P, P, I, I, I, P], I),
    "vrnet_sa_bwd_f32": ([P, L, P, L, P, P, P, P] + [P] * 6 + [P, L] + [P] * 6 + [P, I, L, I, I, I, I, P, L, P], I),
}
for _name, (_args, _res) in _SIGS.items():
    _fn = getattr(_lib, _name)          # AttributeError here = header/library mismatch
    _fn.argtypes = _args
    _fn.restype = _res

if _lib.vrnet_abi_version() != ABI_VERSION:
    raise ImportError(f"libvrnet_hip.so ABI {_lib.vrnet_abi_version()} != expected {ABI_VERSION}")

EXPORTED = tuple(_SIGS)


def _check(rc, name):
    if rc != 0:
        raise RuntimeError(f"{name}: {_lib.vrnet_last_error().decode()}")


class ConvColStats(ctypes.Structure):
    """vrnet_conv_colstats (include/vrnet_hip.h): optional column statistics of a conv's stored outputs."""
    _fields_ = [("partial", P), ("x2", P), ("ldx2", L), ("gamma", P), ("tile_totals", P)]


class PlanesOut(ctypes.Structure):
    """vrnet_planes_out (include/vrnet_hip.h): optional bf16-plane output of a producing kernel."""
    _fields_ = [("p", P), ("ld", L), ("plane", L), ("np", I)]


def _planes_out(pl):
    return None if pl is None else ctypes.byref(PlanesOut(ptr(pl.t), pl.ld, pl.plane, pl.np))


_DTYPES = frozenset((torch.float32, torch.float64, torch.uint8, torch.int64, torch.int32, torch.bfloat16))


def tuning_build():
    """True when the loaded library is the diagnostic build (environment knobs / launch-skipping ablations compiled in)."""
    return bool(_lib.vrnet_tuning_build())


def kernel_launches(family):
    """Launches of a kernel family (codes of last_kernel) by this thread so far."""
    return _lib.vrnet_kernel_launches(family)


def last_kernel():
    """Kernel family of this thread's last conv2d / conv2d_wgrad call (include/vrnet_hip.h)."""
    return _lib.vrnet_last_kernel()


def ptr(t):
    """Device address of a tensor argument.  Every wrapper below passes its tensors through here, so a CPU tensor, an
    unsupported dtype or a view whose innermost stride is not 1 (the kernels take a ROW stride, never an element
    stride) raises instead of handing a meaningless pointer to a kernel."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("vrnet HIP path needs tensors on a HIP device (there is no CPU fallback)")
    if t.dtype not in _DTYPES:
        raise RuntimeError(f"vrnet HIP path: unsupported dtype {t.dtype}")
    if t.dim() and t.stride(-1) != 1 and t.shape[-1] != 1:
        raise RuntimeError(f"vrnet HIP path: innermost dimension must be contiguous (shape {tuple(t.shape)}, "
                           f"strides {t.stride()})")
    return t.data_ptr()


def _tensors(fn, specs):
    """The (tensor or None, shape, dtype) triples of a wrapper's arguments: each tensor contiguous, on the device, of
    exactly that shape and type."""
    for t, sh, dt in specs:
        if t is not None and (t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous() or not t.is_cuda):
            raise RuntimeError(f"{fn}: expected a contiguous {dt} GPU tensor of shape {sh}, got {t.dtype} {tuple(t.shape)}")


def _table_call(fn, geom, replaced=(), table_only=()):
    """Whether this call of a frame op has a geometry table.  The inference-side frame ops are one body each: without geom
    every image fills its slot and the launch arguments carry the geometry; with geom, the (B, GEOM_BYTES) device table of
    `data.frame_geometry`, every image has its own, the `_ragged` entry point runs and flag receives FLAG_GEOMETRY.  The
    `_ragged` names forward to the body, which needs the table then.  replaced: (name, value, default) of the arguments the
    table replaces, absent (at their default) beside a table; table_only: those only a table call has."""
    if geom is None and fn.endswith("_ragged"):
        raise RuntimeError(f"{fn}: the geometry table must be a contiguous, 8-byte aligned uint8 GPU tensor of shape (B, {GEOM_BYTES})")
    clash = [n for n, v, d in (table_only if geom is None else replaced) if not (v is d or (not torch.is_tensor(v) and v == d))]
    if clash:
        raise RuntimeError(f"{fn}: {', '.join(clash)}: " + ("only a call with a geometry table (geom=) takes that" if geom is None else
                                                             "the geometry table holds that for every image; pass it or geom, not both"))
    return geom is not None


def stream():
    return torch.cuda.current_stream().cuda_stream


def empty(*shape, dtype=torch.float32, like=None, device=None):
    return torch.empty(shape, dtype=dtype, device=device if device is not None else like.device)


class Workspace:
    """Grow-only scratch arena (bytes) per (device, stream): kernels on forked streams run concurrently and
    must not share scratch.  Outgrown arenas are retired, never freed: a captured HIP graph may still
    reference them."""

    def __init__(self):
        self.buf = {}
        self.retired = []

    def get(self, nbytes, device):
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            if b is not None:
                self.retired.append(b)
            b = torch.empty(max(int(nbytes) * 2, 8 << 20), dtype=torch.uint8, device=device)
            self.buf[key] = b
        return b


_ws = Workspace()


# --------------------------------------------------------------------------------------- wrappers
def conv2d(a, lda, w, bias, y, ldy, B, H, W, Cin, OH, OW, Cout, kh, kw, stride, pad, dil, mode=0, act=0,
           ypre=None, ldypre=0, res=None, ldres=0, res_scale=None, kscale=None, aux=None, ldaux=0,
           out_nchw=0, out_ctot=0, out_coff=0, accumulate=0, stats=None, precision=0, pair_rows=0, w2=None, bias2=None,
           res_scale2=None, kscale2=None, colstats=None, w_planes=None, workspace=None):
    """pair_rows > 0: two-stream launch, GEMM rows >= pair_rows use (w2, bias2, res_scale2, kscale2).
    colstats = (partial, x2, ldx2, gamma, tile_totals) (None entries allowed): column statistics of the stored outputs.
    workspace (a uint8 tensor): the split workspace of the call, all of it, instead of this stream's scratch arena."""
    cs = None
    if colstats is not None:
        part, x2, ldx2, gam, tot = colstats
        cs = ctypes.byref(ConvColStats(ptr(part), ptr(x2), ldx2, ptr(gam), ptr(tot)))
    # split contraction of the small maps (precision 2): slabs of raw accumulators in this stream's scratch arena
    ws, wsb = None, 0
    if precision == 2:
        rows, cols, ktot = (B * OH * OW, Cout, Cin * kh * kw) if mode == 0 else (B * H * W, Cin, Cout * kh * kw)
        wsb = _lib.vrnet_conv2d_splitk_workspace(rows, cols, ktot)
        if wsb:
            ws = _ws.get(wsb, a.device)
    if workspace is not None:
        ws, wsb = workspace, workspace.numel() * workspace.element_size()
    _check(_lib.vrnet_conv2d_f32(ptr(a), lda, ptr(w), ptr(bias), ptr(y), ldy, B, H, W, Cin, OH, OW, Cout, kh, kw,
                                 stride, pad, dil, mode, act, ptr(ypre), ldypre, ptr(res), ldres, ptr(res_scale),
                                 ptr(kscale), ptr(aux), ldaux, out_nchw, out_ctot, out_coff, accumulate, ptr(stats),
                                 precision, pair_rows, ptr(w2), ptr(bias2), ptr(res_scale2), ptr(kscale2), ptr(w_planes), cs, ptr(ws), wsb, stream()),
           "conv2d")


def conv2d_splitk_workspace(rows, cols, ktot):
    """Bytes of split workspace conv2d gives a precision-2 call of rows x cols over a contraction of ktot (0: no split)."""
    return _lib.vrnet_conv2d_splitk_workspace(rows, cols, ktot)


def conv_planes_bytes(J, K):
    return _lib.vrnet_conv_planes_bytes(J, K)


def conv_planes_pack(table, nentries, total_blocks):
    """table: int64 device tensor, 8 values per entry (vrnet_conv_planes_pack_f32)."""
    _check(_lib.vrnet_conv_planes_pack_f32(ptr(table), nentries, total_blocks, stream()), "conv_planes_pack")


# ---- plane tensors (csrc/pgemm.hip): an fp32 tensor as three bf16 planes, t = p0 + p1 + p2 exactly, or (np = 1) a bf16 tensor
class Planes:
    """bf16 planes of a (rows, C) matrix: `t` is a (np, ..., C) bfloat16 tensor, plane q = t[q]; `ld` row stride, `plane`
    plane stride (elements).  np = 3: the fp32 values, exactly (float(t).sum(0) in the order p2 + p1 + p0 reproduces them);
    np = 1: the values rounded to bf16."""
    __slots__ = ("t", "np", "ld", "plane", "C")

    def __init__(self, t, ld=None, plane=None):
        assert t.dtype == torch.bfloat16 and t.stride(-1) == 1
        self.t, self.np, self.C = t, t.shape[0], t.shape[-1]
        self.ld = t.stride(-2) if ld is None else ld
        self.plane = t.stride(0) if plane is None else plane

    @staticmethod
    def empty(np_, shape, device):
        return Planes(torch.empty((np_,) + tuple(shape), dtype=torch.bfloat16, device=device))

    def float(self):
        """The fp32 tensor the planes stand for (exact for np = 3)."""
        f = self.t.float()
        return f[0] if self.np == 1 else (f[2] + f[1]) + f[0]


def gemm_planes_ok(rows, cols, K):
    """Whether gemm_planes has a kernel for a rows x cols product over a contraction of K."""
    return bool(_lib.vrnet_gemm_planes_ok(rows, cols, K))


def gemm_planes(a, b, M, N, K, bias=None, y=None, ldy=0, yp=None, act=0, ypre=None, ldypre=0, res=None, ldres=0,
                res_scale=None, aux=None, ldaux=0, accumulate=0, stats=None, stats_hw=0, colstats=None):
    """y / yp = epilogue(A . B^T) on plane operands a, b (Planes, same np); y: fp32 tensor or None, yp: Planes or None.
    ypre / aux may be bfloat16 tensors (the Mlp's pre-activation in bf16 mode; strides in elements)."""
    assert a.np == b.np
    half_side = (1 if (ypre is not None and ypre.dtype == torch.bfloat16) else 0) | \
        (2 if (aux is not None and aux.dtype == torch.bfloat16) else 0)
    cs = None
    if colstats is not None:
        part, x2, ldx2, gam, tot = colstats
        cs = ctypes.byref(ConvColStats(ptr(part), ptr(x2), ldx2, ptr(gam), ptr(tot)))
    _check(_lib.vrnet_gemm_planes_f32(ptr(a.t), a.ld, a.plane, ptr(b.t), b.ld, b.plane, a.np, M, N, K, ptr(bias), ptr(y), ldy,
                                      None if yp is None else ptr(yp.t), 0 if yp is None else yp.ld,
                                      0 if yp is None else yp.plane, 0 if yp is None else yp.np, act, ptr(ypre), ldypre,
                                      ptr(res), ldres, ptr(res_scale), ptr(aux), ldaux, accumulate, ptr(stats), stats_hw, cs,
                                      half_side, stream()), "gemm_planes")


def planes_split_blocks(R, K):
    return _lib.vrnet_planes_split_blocks(R, K)


def planes_split(table, nentries, total_blocks, np_):
    """table: int64 device tensor, 10 values per entry (vrnet_planes_split_f32)."""
    _check(_lib.vrnet_planes_split_f32(ptr(table), nentries, total_blocks, np_, stream()), "planes_split")


def planes_from_f32(src, lds, R, K, out):
    """out (Planes) = the row-major fp32 matrix `src` (R rows of K values, row stride lds)."""
    _check(_lib.vrnet_planes_from_f32(ptr(src), lds, R, K, ptr(out.t), out.ld, out.plane, out.np, stream()), "planes_from_f32")


def wgrad_planes_ok(M, Cin, Cout):
    return bool(_lib.vrnet_wgrad_planes_ok(M, Cin, Cout))


def wgrad_planes_plan(M, Cin, Cout, np_):
    """(n_tiles, c_tiles, splits, rows_per_split) of wgrad_planes at np_ = 3 or 1 (vrnet_wgrad_planes_plan; a host call)."""
    out = [ctypes.c_int() for _ in range(4)]
    _check(_lib.vrnet_wgrad_planes_plan(M, Cin, Cout, np_, *(ctypes.byref(o) for o in out)), "wgrad_planes_plan")
    return tuple(o.value for o in out)


def wgrad_planes_workspace(M, Cin, Cout):
    """Bytes of workspace wgrad_planes needs (either np)."""
    return _lib.vrnet_wgrad_planes_workspace(M, Cin, Cout)


def wgrad_planes(x, dy, M, Cin, Cout, dw, dbias=None, row_scale=None, accumulate=0, w=None, bias=None, dls=None, ws=None,
                 ws_bytes=None):
    """dw (+ dbias, + dls) of a 1x1 conv from plane operands x (M x Cin) and dy (M x Cout) (vrnet_wgrad_planes_f32).
    ws (a tensor): the workspace of the call instead of this stream's scratch arena; ws_bytes: how much of it the call may use
    (default: all of it)."""
    assert x.np == dy.np
    if ws is None:
        ws = _ws.get(_lib.vrnet_wgrad_planes_workspace(M, Cin, Cout), dw.device)
    if ws_bytes is None:
        ws_bytes = ws.numel() * ws.element_size()
    _check(_lib.vrnet_wgrad_planes_f32(ptr(x.t), x.ld, x.plane, ptr(dy.t), dy.ld, dy.plane, x.np, M, Cin, Cout, ptr(dw), ptr(dbias),
                                       ptr(row_scale), accumulate, ptr(w), ptr(bias), ptr(dls), ptr(ws), ws_bytes, stream()),
           "wgrad_planes")


def bf16_conv_ok(lda, Cin, Cout, mode):
    """Shapes the bf16-operand path of conv2d accepts (mirrors the check in vrnet_conv2d_f32)."""
    ck, cn = (Cin, Cout) if mode == 0 else (Cout, Cin)
    return ck % 4 == 0 and lda % 4 == 0 and cn > 32 and cn % 4 == 0


def conv2d_dma_tile(rows, cols):
    """22 / 21 / 0: tile of the LDS-DMA x6 / bf16 kernels for a GEMM of rows x cols (0 = no such kernel)."""
    return _lib.vrnet_conv2d_dma_tile(rows, cols)


def conv2d_dma_plan(rows, cols, ktot):
    """(tile, splits) of conv2d at precision 2 for a GEMM of rows x cols with a contraction of ktot: the unsplit tile with
    splits = 1, or tile 21 with the K loop split over `splits` workgroups per tile (small maps), or (0, 1)."""
    s = ctypes.c_int(1)
    t = _lib.vrnet_conv2d_dma_plan(rows, cols, ktot, ctypes.byref(s))
    return t, s.value


def pack_weight_t(w_oihw, kscale, out, Cout, Cin, kh, kw):
    _check(_lib.vrnet_pack_weight_t_f32(ptr(w_oihw), ptr(kscale), ptr(out), Cout, Cin, kh, kw, stream()), "pack_weight_t")


def conv_stats_buffer(B, HW, Cout, device):
    """(buffer, pairs per sample) for the `stats` output of conv2d, or (None, 0) when the shape does not qualify."""
    if HW % 32 or Cout <= 32 or Cout % 4:
        return None, 0
    nb = (Cout + 31) // 32
    return torch.empty((B * HW // 32, nb, 2), dtype=torch.float64, device=device), (HW // 32) * nb


def conv2d_wgrad(x, ldx, dy, lddy, dw, dbias, row_scale, B, H, W, Cin, OH, OW, Cout, kh, kw, stride, pad, dil,
                 accumulate=0, precision=0, dw2=None, dbias2=None, row_scale2=None, w=None, bias=None, dls=None,
                 w2=None, bias2=None, dls2=None):
    """dw2 given: two-stream launch, samples [B/2, B) contribute to (dw2, dbias2, row_scale2).
    dls given (1x1 convs): layer-scale gradient rowdot(w, dw_raw) + bias * db_raw."""
    nbytes = _lib.vrnet_conv2d_wgrad_workspace(B, OH, OW, Cin, Cout, kh, kw, 1 if dw2 is not None else 0)
    ws = _ws.get(nbytes, x.device)
    _check(_lib.vrnet_conv2d_wgrad_f32(ptr(x), ldx, ptr(dy), lddy, ptr(dw), ptr(dbias), ptr(row_scale), B, H, W, Cin,
                                       OH, OW, Cout, kh, kw, stride, pad, dil, accumulate, precision, ptr(dw2),
                                       ptr(dbias2), ptr(row_scale2), ptr(w), ptr(bias), ptr(dls), ptr(w2), ptr(bias2),
                                       ptr(dls2), ptr(ws), ws.numel(), stream()), "conv2d_wgrad")


def conv2d_wgrad_plan(rows, Cin, Cout, taps, ident, vec, precision=0, has_bias=True, has_dls=False):
    """(kernel, tile, S, rows_per_split, xcd_group, reduce, VEC, SL) of conv2d_wgrad's MFMA path for `rows` output pixels per
    stream (vrnet_conv2d_wgrad_plan in include/vrnet_hip.h; a host call).  Raises where conv2d_wgrad refuses the call."""
    out = (ctypes.c_int * 8)()
    _check(_lib.vrnet_conv2d_wgrad_plan(rows, Cin, Cout, taps, int(ident), int(vec), precision, int(has_bias), int(has_dls), out),
           "conv2d_wgrad_plan")
    return tuple(out)


CONV_PLAN_FLAGS = dict(a=1, w=2, y=4, bias=8, ypre=16, res=32, res_scale=64, aux=128)


def conv2d_plan(B, H, W, Cin, OH, OW, Cout, kh, kw, stride, pad, dil, mode=0, precision=0, lda=None, ldy=None, misaligned=(),
                kscale=False, plain=False, out_nchw=False, stats=False, colstats=False, w_planes=False, workspace_bytes=0):
    """(family, kernel, tile, S, k_live, perm2, a_vec, b_vec, e_vec, grid x, grid y, finish grid) of a single-stream conv2d call
    (vrnet_conv2d_plan in include/vrnet_hip.h; a host call).  lda, ldy default to the channel counts; misaligned: names of
    CONV_PLAN_FLAGS whose operand is given and not on 16-byte rows; plain: no fused epilogue operand (ypre, res, kscale, aux,
    act).  Raises where conv2d refuses the call."""
    ck, cn = (Cin, Cout) if mode == 0 else (Cout, Cin)
    flags = sum(v for k, v in CONV_PLAN_FLAGS.items() if k not in misaligned)
    flags |= 256 * bool(kscale) | 512 * bool(plain) | 1024 * bool(out_nchw) | 2048 * bool(stats) | 4096 * bool(colstats) | 8192 * bool(w_planes)
    out = (ctypes.c_int * 12)()
    _check(_lib.vrnet_conv2d_plan(B, H, W, Cin, OH, OW, Cout, kh, kw, stride, pad, dil, mode, precision, ck if lda is None else lda,
                                  cn if ldy is None else ldy, flags, workspace_bytes, out), "conv2d_plan")
    return tuple(out)


def bf16_wgrad_ok(ldx, lddy, Cin, Cout):
    return Cin % 4 == 0 and Cout % 4 == 0 and ldx % 4 == 0 and lddy % 4 == 0 and Cin > 32 and Cout > 32


def pack_weight(w_oihw, out, Cout, Cin, kh, kw):
    _check(_lib.vrnet_pack_weight_f32(ptr(w_oihw), ptr(out), Cout, Cin, kh, kw, stream()), "pack_weight")


def mlp_fused_ok(C, HID, M):
    """Whether the fused fc1 -> GELU -> fc2 kernels exist for block width C, hidden width HID and M rows."""
    return bool(_lib.vrnet_mlp_fused_ok(C, HID, M))


def mlp_pack(w1, w2, C, HID, precision, want_bwd=True):
    """(forward planes, backward planes) of an Mlp's weights: bf16 planes in MFMA fragment order (vrnet_mlp_pack_f32)."""
    n = _lib.vrnet_mlp_pack_bytes(C, HID, precision)
    fwd = torch.empty((n,), dtype=torch.uint8, device=w1.device)
    bwd = torch.empty((n,), dtype=torch.uint8, device=w1.device) if want_bwd else None
    _check(_lib.vrnet_mlp_pack_f32(ptr(w1), ptr(w2), C, HID, precision, ptr(fwd), ptr(bwd), stream()), "mlp_pack")
    return fwd, bwd


def mlp_rc_ok(C, HID, M=32):
    """Whether the recompute form of the fused Mlp backward (mlp_bwd_rc) exists for this block (the library's own predicate:
    vrnet_mlp_rc_ok, which vrnet_mlp_pack_rc_f32 and vrnet_mlp_bwd_rc_f32 check too)."""
    return bool(_lib.vrnet_mlp_rc_ok(C, HID, M))


def mlp_pack_rc(w1, w2, C, HID, precision):
    """Planes of the backward kernel that recomputes the pre-activation: per chunk [fc2^T | fc1^T | fc1]."""
    pack = torch.empty((_lib.vrnet_mlp_pack_rc_bytes(C, HID, precision),), dtype=torch.uint8, device=w1.device)
    _check(_lib.vrnet_mlp_pack_rc_f32(ptr(w1), ptr(w2), C, HID, precision, ptr(pack), stream()), "mlp_pack_rc")
    return pack


def mlp_bwd_rc(dy, lddy, dy_scale, pack, x, ldx, b1, h, ldh, du, lddu, dx, lddx, M, C, HID, precision):
    _check(_lib.vrnet_mlp_bwd_rc_f32(ptr(dy), lddy, ptr(dy_scale), ptr(pack), ptr(x), ldx, ptr(b1), ptr(h), ldh, ptr(du), lddu,
                                     ptr(dx), lddx, M, C, HID, precision, stream()), "mlp_bwd_rc")


def mlp_fwd(x, ldx, pack, b1, b2, res, ldres, res_scale, y, ldy, upre, ldu, stats, M, C, HID, precision):
    _check(_lib.vrnet_mlp_fwd_f32(ptr(x), ldx, ptr(pack), ptr(b1), ptr(b2), ptr(res), ldres, ptr(res_scale), ptr(y), ldy,
                                  ptr(upre), ldu, ptr(stats), M, C, HID, precision, stream()), "mlp_fwd")


def mlp_bwd(dy, lddy, dy_scale, pack, upre, ldu, h, ldh, du, lddu, dx, lddx, M, C, HID, precision):
    _check(_lib.vrnet_mlp_bwd_f32(ptr(dy), lddy, ptr(dy_scale), ptr(pack), ptr(upre), ldu, ptr(h), ldh, ptr(du), lddu,
                                  ptr(dx), lddx, M, C, HID, precision, stream()), "mlp_bwd")


def moments(x, ldx, B, HW, C, x2=None, ldx2=0, mask=None, ldm=0, out=None):
    if out is None:
        out = torch.empty((B, C, 2), dtype=torch.float64, device=x.device)
    ws = _ws.get(_lib.vrnet_moments_workspace(B, HW, C), x.device)
    _check(_lib.vrnet_moments_f32(ptr(x), ldx, ptr(x2), ldx2, ptr(mask), ldm, B, HW, C, ptr(out), ptr(ws), ws.numel(),
                                  stream()), "moments")
    return out


def affine(out, ldo, B, HW, C, x1=None, ld1=0, A=None, D1=None, pre=0, masky=None, ldm=0, x2=None, ld2=0, E=None,
           D2=None, bstride=0, accumulate=0, S1=None, S2=None, add=None, ldadd=0):
    """out = pre(A*(x1-S1)+D1) + E*(x2-S2) + D2 [+ out (accumulate=1) | + add (out of place)]."""
    _check(_lib.vrnet_affine_f32(ptr(x1), ld1, ptr(A), ptr(D1), ptr(S1), pre, ptr(masky), ldm, ptr(x2), ld2, ptr(E),
                                 ptr(D2), ptr(S2), bstride, ptr(out), ldo, B, HW, C, accumulate, ptr(add), ldadd, stream()),
           "affine")


def gn_coef_fwd(mom, gamma, beta, eps, B, HW, C, A, Dc, S, mean_rstd):
    _check(_lib.vrnet_gn_coef_fwd(ptr(mom), ptr(gamma), ptr(beta), eps, B, HW, C, ptr(A), ptr(Dc), ptr(S),
                                  ptr(mean_rstd), stream()), "gn_coef_fwd")


def gn_coef_from_pairs(pairs, per_sample, gamma, beta, eps, B, HW, C, A, Dc, S, mean_rstd, gamma2=None, beta2=None):
    _check(_lib.vrnet_gn_coef_from_pairs(ptr(pairs), per_sample, ptr(gamma), ptr(beta), eps, B, HW, C, ptr(A), ptr(Dc),
                                         ptr(S), ptr(mean_rstd), ptr(gamma2), ptr(beta2), stream()), "gn_coef_from_pairs")


def gn_stats_fwd(x, ldx, gamma, beta, eps, B, HW, C, A, Dc, S, mean_rstd, gamma2=None, beta2=None):
    ws = _ws.get(_lib.vrnet_moments_workspace(B, HW, C), x.device)
    _check(_lib.vrnet_gn_stats_fwd(ptr(x), ldx, ptr(gamma), ptr(beta), eps, B, HW, C, ptr(A), ptr(Dc), ptr(S),
                                   ptr(mean_rstd), ptr(gamma2), ptr(beta2), ptr(ws), ws.numel(), stream()), "gn_stats_fwd")


def gn_apply_ok(C, *lds):
    """Shapes the one-launch GroupNorm kernels accept: C % 4 == 0 and row strides that are multiples of 4."""
    return C % 4 == 0 and all(ld % 4 == 0 for ld in lds)


def gn_apply_fwd(x, ldx, pairs, per_sample, gamma, beta, eps, B, HW, C, y, ldy, mean_rstd, planes=None):
    """planes (Planes): the result also (y given) or only (y None) as bf16 planes."""
    if planes is None:
        _check(_lib.vrnet_gn_apply_fwd(ptr(x), ldx, ptr(pairs), per_sample, ptr(gamma), ptr(beta), eps, B, HW, C, ptr(y), ldy,
                                       ptr(mean_rstd), stream()), "gn_apply_fwd")
    else:
        _check(_lib.vrnet_gn_apply_fwd_planes(ptr(x), ldx, ptr(pairs), per_sample, ptr(gamma), ptr(beta), eps, B, HW, C, ptr(y), ldy,
                                              ptr(mean_rstd), _planes_out(planes), stream()), "gn_apply_fwd_planes")


def gn_apply_bwd(dy, lddy, x, ldx, mean_rstd, gamma, B, HW, C, out, ldo, dgamma, dbeta, accumulate_params, add=None, ldadd=0,
                 planes=None):
    ws = _ws.get(_lib.vrnet_gn_bwd_workspace(B, HW, C), x.device)
    if planes is None:
        _check(_lib.vrnet_gn_apply_bwd(ptr(dy), lddy, ptr(x), ldx, ptr(mean_rstd), ptr(gamma), B, HW, C, ptr(add), ldadd, ptr(out),
                                       ldo, ptr(dgamma), ptr(dbeta), accumulate_params, ptr(ws), ws.numel(), stream()), "gn_apply_bwd")
    else:
        _check(_lib.vrnet_gn_apply_bwd_planes(ptr(dy), lddy, ptr(x), ldx, ptr(mean_rstd), ptr(gamma), B, HW, C, ptr(add), ldadd,
                                              ptr(out), ldo, ptr(dgamma), ptr(dbeta), accumulate_params, _planes_out(planes),
                                              ptr(ws), ws.numel(), stream()), "gn_apply_bwd_planes")


def colstats_ok(HW, Cout, *lds):
    """Shapes for which a conv can leave the column statistics of its output (see conv2d `colstats`)."""
    return HW % 32 == 0 and Cout > 32 and Cout % 4 == 0 and all(ld % 4 == 0 for ld in lds)


def colstats_buffers(B, HW, C, device, totals=False):
    part = torch.empty((B * HW // 32, C, 2), dtype=torch.float64, device=device)
    tot = torch.empty((B * HW // 32, (C + 31) // 32, 2), dtype=torch.float64, device=device) if totals else None
    return part, tot


def gn_apply_bwd_from_partials(dy, lddy, x, ldx, partial, tile_totals, mean_rstd, gamma, B, HW, C, out, ldo, dgamma, dbeta,
                               accumulate_params, add=None, ldadd=0):
    _check(_lib.vrnet_gn_apply_bwd_from_partials(ptr(dy), lddy, ptr(x), ldx, ptr(partial), ptr(tile_totals), ptr(mean_rstd),
                                                 ptr(gamma), B, HW, C, ptr(add), ldadd, ptr(out), ldo, ptr(dgamma), ptr(dbeta),
                                                 accumulate_params, stream()), "gn_apply_bwd_from_partials")


def bn_coef_fwd_from_partials(partial, gamma, beta, eps, momentum, rm, rv, nbt, B, HW, C, A, Dc, S, mean_rstd):
    _check(_lib.vrnet_bn_coef_fwd_from_partials(ptr(partial), ptr(gamma), ptr(beta), eps, momentum, ptr(rm), ptr(rv), ptr(nbt), B,
                                                HW, C, ptr(A), ptr(Dc), ptr(S), ptr(mean_rstd), stream()), "bn_coef_fwd_from_partials")


def gn_coef_bwd(mom2, mean_rstd, gamma, B, HW, C, A, E, Dc, S, dgamma, dbeta, accumulate, gamma2=None, dgamma2=None,
                dbeta2=None):
    _check(_lib.vrnet_gn_coef_bwd(ptr(mom2), ptr(mean_rstd), ptr(gamma), B, HW, C, ptr(A), ptr(E), ptr(Dc), ptr(S),
                                  ptr(dgamma), ptr(dbeta), accumulate, ptr(gamma2), ptr(dgamma2), ptr(dbeta2), stream()),
           "gn_coef_bwd")


def bn_coef_fwd(mom, gamma, beta, eps, momentum, rm, rv, nbt, training, B, HW, C, A, Dc, S, mean_rstd):
    _check(_lib.vrnet_bn_coef_fwd(ptr(mom), ptr(gamma), ptr(beta), eps, momentum, ptr(rm), ptr(rv), ptr(nbt),
                                  int(training), B, HW, C, ptr(A), ptr(Dc), ptr(S), ptr(mean_rstd), stream()),
           "bn_coef_fwd")


def bn_coef_bwd(mom2, mean_rstd, gamma, training, B, HW, C, A, E, Dc, S, dgamma, dbeta, accumulate):
    _check(_lib.vrnet_bn_coef_bwd(ptr(mom2), ptr(mean_rstd), ptr(gamma), int(training), B, HW, C, ptr(A), ptr(E),
                                  ptr(Dc), ptr(S), ptr(dgamma), ptr(dbeta), accumulate, stream()), "bn_coef_bwd")


def bn_stats_fwd(x, ldx, gamma, beta, eps, momentum, rm, rv, nbt, B, HW, C, A, Dc, S, mean_rstd):
    """Train-mode BatchNorm: batch moments of x + coefficients + running statistics in two launches."""
    ws = _ws.get(_lib.vrnet_moments_workspace(B, HW, C), x.device)
    _check(_lib.vrnet_bn_stats_fwd(ptr(x), ldx, ptr(gamma), ptr(beta), eps, momentum, ptr(rm), ptr(rv), ptr(nbt), B, HW, C,
                                   ptr(A), ptr(Dc), ptr(S), ptr(mean_rstd), ptr(ws), ws.numel(), stream()), "bn_stats_fwd")


def bn_stats_bwd(dy, lddy, z, ldz, mask, ldm, mean_rstd, gamma, training, B, HW, C, A, E, Dc, S, dgamma, dbeta, accumulate):
    ws = _ws.get(_lib.vrnet_moments_workspace(B, HW, C), dy.device)
    _check(_lib.vrnet_bn_stats_bwd(ptr(dy), lddy, ptr(z), ldz, ptr(mask), ldm, ptr(mean_rstd), ptr(gamma), int(training), B,
                                   HW, C, ptr(A), ptr(E), ptr(Dc), ptr(S), ptr(dgamma), ptr(dbeta), accumulate, ptr(ws),
                                   ws.numel(), stream()), "bn_stats_bwd")


def bn_stats_bwd_zmask(dy, lddy, z, ldz, fwd, mean_rstd, gamma, training, B, HW, C, A, E, Dc, S, dgamma, dbeta, accumulate):
    """bn_stats_bwd with the ReLU mask recomputed from z: fwd = the forward apply's (A, D, S)."""
    ws = _ws.get(_lib.vrnet_moments_workspace(B, HW, C), dy.device)
    _check(_lib.vrnet_bn_stats_bwd_zmask(ptr(dy), lddy, ptr(z), ldz, ptr(fwd[0]), ptr(fwd[1]), ptr(fwd[2]), ptr(mean_rstd),
                                         ptr(gamma), int(training), B, HW, C, ptr(A), ptr(E), ptr(Dc), ptr(S), ptr(dgamma),
                                         ptr(dbeta), accumulate, ptr(ws), ws.numel(), stream()), "bn_stats_bwd_zmask")


def bn_apply_bwd_zmask(dy, lddy, z, ldz, fwd, A, E, Dc, S, dz, lddz, B, HW, C):
    _check(_lib.vrnet_bn_apply_bwd_zmask(ptr(dy), lddy, ptr(z), ldz, ptr(fwd[0]), ptr(fwd[1]), ptr(fwd[2]), ptr(A), ptr(E),
                                         ptr(Dc), ptr(S), ptr(dz), lddz, B, HW, C, stream()), "bn_apply_bwd_zmask")


def eca_coef_fwd(mom, wk, k, B, HW, C, gate):
    _check(_lib.vrnet_eca_coef_fwd(ptr(mom), ptr(wk), k, B, HW, C, ptr(gate), stream()), "eca_coef_fwd")


def eca_coef_bwd(mom2, mom, gate, wk, k, B, HW, C, Fc, dwk, accumulate):
    _check(_lib.vrnet_eca_coef_bwd(ptr(mom2), ptr(mom), ptr(gate), ptr(wk), k, B, HW, C, ptr(Fc), ptr(dwk), accumulate,
                                   stream()), "eca_coef_bwd")


def ls_coef_bwd(mom2, ls, B, C, dls, dbias, accumulate, pair=0, ls2=None, dls2=None, dbias2=None):
    _check(_lib.vrnet_ls_coef_bwd(ptr(mom2), ptr(ls), B, C, ptr(dls), ptr(dbias), accumulate, pair, ptr(ls2), ptr(dls2),
                                  ptr(dbias2), stream()), "ls_coef_bwd")


def moments_to_float(mom, out, n, scale, which=0):
    _check(_lib.vrnet_moments_to_float(ptr(mom), ptr(out), n, scale, which, stream()), "moments_to_float")


def patch_gather(x, ldx, pos, out, B, H, W, C, CP, k):
    _check(_lib.vrnet_patch_gather_f32(ptr(x), ldx, ptr(pos), ptr(out), B, H, W, C, CP, k, stream()), "patch_gather")


def patch_scatter(dp, dx, lddx, B, H, W, C, CP, k, accumulate=0):
    _check(_lib.vrnet_patch_scatter_f32(ptr(dp), ptr(dx), lddx, B, H, W, C, CP, k, accumulate, stream()), "patch_scatter")


def weight_ohwi(src, dst, Cout, Cin, kh, kw, direction, accumulate=0):
    _check(_lib.vrnet_weight_ohwi_f32(ptr(src), ptr(dst), Cout, Cin, kh, kw, direction, accumulate, stream()), "weight_ohwi")


def copy_channels(src, lds, scs, dst, ldd, dcs, rows, C, accumulate=0):
    _check(_lib.vrnet_copy_channels_f32(ptr(src), lds, scs, ptr(dst), ldd, dcs, rows, C, accumulate, stream()),
           "copy_channels")


def cat2(a, lda, Ca, b, ldb, Cb, cat, ldc, rows, interleave, dir=0, accumulate_a=0, accumulate_b=0):
    """dir 0: cat = torch.cat([a, b], channels) (+ 2-group shuffle when interleave); dir 1: the adjoint (a / b may be None)."""
    _check(_lib.vrnet_cat2_f32(ptr(a), lda, Ca, ptr(b), ldb, Cb, ptr(cat), ldc, rows, int(interleave), dir, accumulate_a,
                               accumulate_b, stream()), "cat2")


def nchw_to_nhwc(src, dst, ldd, B, C, HW):
    _check(_lib.vrnet_nchw_to_nhwc_f32(ptr(src), ptr(dst), ldd, B, C, HW, stream()), "nchw_to_nhwc")


def nhwc_to_nchw(src, lds, dst, B, C, HW, accumulate=0):
    _check(_lib.vrnet_nhwc_to_nchw_f32(ptr(src), lds, ptr(dst), B, C, HW, accumulate, stream()), "nhwc_to_nchw")


def add_(dst, src):
    _check(_lib.vrnet_add_f32(ptr(dst), ptr(src), dst.numel(), stream()), "add")


def clock_stamp(buf, slot):
    """buf[slot] (int64) = the device clock (100 MHz) when the stream reaches this point (diagnostic)."""
    _check(_lib.vrnet_clock_stamp(buf.data_ptr() + 8 * slot, stream()), "clock_stamp")


def fill_(dst, value):
    _check(_lib.vrnet_fill_f32(ptr(dst), float(value), dst.numel(), stream()), "fill")


def cluster_state_floats(B, H, W, E, fold):
    """Floats of per-region forward state for regions of more than 256 points (0: none needed)."""
    return _lib.vrnet_cluster_state_floats(B, H, W, E, fold)


def cluster_plan(N, blocks, bwd):
    """(T, NPT) of the register kernel a Cluster launch on regions of N points in `blocks` = B * E * fold^2 workgroups runs,
    (0, 0) for the streaming kernel (vrnet_cluster_plan in include/vrnet_hip.h; a host call).  Raises where the launch is refused."""
    T, npt = ctypes.c_int(-1), ctypes.c_int(-1)
    _check(_lib.vrnet_cluster_plan(N, blocks, int(bool(bwd)), ctypes.byref(T), ctypes.byref(npt)), "cluster_plan")
    return T.value, npt.value


def cluster_fwd(f, v, ld, alpha, beta, out, ldo, idx, wgt, B, H, W, E, Dh, fold, alpha2=None, beta2=None, forced=False,
                planes=None, state=None):
    """forced: idx is given (read), not computed (teacher-forced assignment for parity comparisons).
    planes (Planes): `out` as bf16 planes, beside the fp32 `out` or instead of it (out None); single-stream launches.
    f / v may then be bfloat16 tensors (ld in elements).  state (cluster_state_floats floats): the forward's per-region state
    for cluster_bwd(saved=(wgt, state))."""
    if planes is not None or f.dtype == torch.bfloat16 or state is not None:
        assert alpha2 is None and f.dtype == v.dtype
        _check(_lib.vrnet_cluster_fwd_planes_f32(ptr(f), ptr(v), ld, 1 if f.dtype == torch.bfloat16 else 0, ptr(alpha), ptr(beta),
                                                 ptr(out), ldo, ptr(idx), ptr(wgt), B, H, W, E, Dh, fold, 1 if forced else 0,
                                                 _planes_out(planes), ptr(state), stream()), "cluster_fwd_planes")
        return
    fn = _lib.vrnet_cluster_fwd_forced_f32 if forced else _lib.vrnet_cluster_fwd_f32
    _check(fn(ptr(f), ptr(v), ld, ptr(alpha), ptr(beta), ptr(out), ldo, ptr(idx), ptr(wgt), B, H,
                                      W, E, Dh, fold, ptr(alpha2), ptr(beta2), stream()), "cluster_fwd")


def cluster_bwd(f, v, ld, alpha, beta, idx, dout, lddo, df, dv, lddf, dalpha, dbeta, accumulate_ab, B, H, W, E, Dh,
                fold, alpha2=None, beta2=None, dalpha2=None, dbeta2=None, planes=None, saved=None):
    """planes (Planes of 2 E Dh columns): a second copy of [df | dv] as bf16 planes (single-stream launches).
    saved = (wgt, state) of the forward (regions of more than 256 points): the backward skips its first two passes."""
    nb = _lib.vrnet_cluster_bwd_workspace2(B, H, W, E, fold)
    # dalpha is None: the (d alpha, d beta) partials stay in the workspace -- then a buffer of its own, returned to the caller,
    # who reduces a whole section's modules with one cluster_ab_reduce_multi
    ws = torch.empty(nb, dtype=torch.uint8, device=f.device) if dalpha is None else _ws.get(nb, f.device)
    if planes is not None or f.dtype == torch.bfloat16 or saved is not None or dalpha is None:
        assert alpha2 is None and f.dtype == v.dtype == dout.dtype
        wf, st = saved if saved is not None else (None, None)
        _check(_lib.vrnet_cluster_bwd_planes_f32(ptr(f), ptr(v), ld, 1 if f.dtype == torch.bfloat16 else 0, ptr(alpha), ptr(beta),
                                                 ptr(idx), ptr(dout), lddo, ptr(df), ptr(dv), lddf, ptr(dalpha), ptr(dbeta),
                                                 accumulate_ab, B, H, W, E, Dh, fold, _planes_out(planes), ptr(wf), ptr(st),
                                                 ptr(ws), ws.numel(), stream()), "cluster_bwd_planes")
        return ws if dalpha is None else None
    _check(_lib.vrnet_cluster_bwd_f32(ptr(f), ptr(v), ld, ptr(alpha), ptr(beta), ptr(idx), ptr(dout), lddo, ptr(df),
                                      ptr(dv), lddf, ptr(dalpha), ptr(dbeta), accumulate_ab, B, H, W, E, Dh, fold,
                                      ptr(alpha2), ptr(beta2), ptr(dalpha2), ptr(dbeta2), ptr(ws), ws.numel(), stream()),
           "cluster_bwd")


def cluster_ab_reduce_multi(entries):
    """entries: [(workspace a deferred cluster_bwd returned, B * E * fold^2, dalpha, dbeta, accumulate)]: ONE launch."""
    n = len(entries)
    PA, LA, IA = ctypes.c_void_p * n, ctypes.c_long * n, ctypes.c_int * n
    _check(_lib.vrnet_cluster_ab_reduce_multi(n, PA(*[ptr(e[0]) for e in entries]), LA(*[int(e[1]) for e in entries]),
                                              PA(*[ptr(e[2]) for e in entries]), PA(*[ptr(e[3]) for e in entries]),
                                              IA(*[int(e[4]) for e in entries]), stream()), "cluster_ab_reduce_multi")


def dwconv3x3(x, ldx, w, y, ldy, B, H, W, C, flip=0, accumulate=0):
    _check(_lib.vrnet_dwconv3x3_f32(ptr(x), ldx, ptr(w), ptr(y), ldy, B, H, W, C, flip, accumulate, stream()),
           "dwconv3x3")


def dwconv3x3_wgrad(x, ldx, dy, lddy, dw, B, H, W, C, accumulate=0):
    ws = _ws.get(_lib.vrnet_dwconv3x3_wgrad_workspace(B, H, W, C), x.device)
    _check(_lib.vrnet_dwconv3x3_wgrad_f32(ptr(x), ldx, ptr(dy), lddy, ptr(dw), B, H, W, C, accumulate, ptr(ws),
                                          ws.numel(), stream()), "dwconv3x3_wgrad")


def upsample(x, ldx, y, ldy, B, H, W, C, scale, out_nchw=0):
    _check(_lib.vrnet_upsample_bilinear_f32(ptr(x), ldx, ptr(y), ldy, B, H, W, C, scale, out_nchw, stream()),
           "upsample")


def bn_relu_upsample(z, ldz, A, Dc, S, y, ldy, B, H, W, C, scale, out_nchw=0):
    """y = upsample(ReLU(A (z - S) + Dc)): BatchNorm apply + ReLU on the taps (CoCUpsample without its low-resolution output)."""
    _check(_lib.vrnet_bn_relu_upsample_bilinear_f32(ptr(z), ldz, ptr(A), ptr(Dc), ptr(S), ptr(y), ldy, B, H, W, C, scale, out_nchw,
                                                    stream()), "bn_relu_upsample")


def upsample_bwd(dy, lddy, dy_nchw, dx, lddx, B, H, W, C, scale, accumulate=0):
    _check(_lib.vrnet_upsample_bilinear_bwd_f32(ptr(dy), lddy, dy_nchw, ptr(dx), lddx, B, H, W, C, scale, accumulate,
                                                stream()), "upsample_bwd")


def upsample_bwd_cat(dy, lddy, coff, cstride, dx, lddx, B, H, W, C, scale, accumulate=0):
    """upsample_bwd with its NHWC dy read in place from a concatenation's gradient: channel j at column coff + cstride * j."""
    _check(_lib.vrnet_upsample_bilinear_bwd_cat_f32(ptr(dy), lddy, coff, cstride, ptr(dx), lddx, B, H, W, C, scale, accumulate,
                                                    stream()), "upsample_bwd_cat")


def up_cat_ok(C, Cs, ldz, lds, ldc, interleave, *tensors):
    """Shapes bn_relu_upsample_cat takes: channel counts and row strides % 4 (equal widths with the shuffle), 16-byte aligned bases."""
    return bool(_lib.vrnet_up_cat_ok(C, Cs, ldz, lds, ldc, int(interleave))) and all(t.data_ptr() % 16 == 0 for t in tensors)


UP_CAT_NONE, UP_CAT_SA_SUMS, UP_CAT_GN_PAIRS = 0, 1, 2


def bn_relu_upsample_cat(z, ldz, A, Dc, S, skip, lds, cat, ldc, B, H, W, C, Cs, scale, up_first, interleave, stats=UP_CAT_NONE):
    """cat = torch.cat of upsample(ReLU(A (z - S) + Dc)) (A None: of upsample(z)) and skip, [up | skip] if up_first else
    [skip | up], + the 2-group channel shuffle when interleave -- one launch, the interpolated map is never stored.
    Returns None, the (B, C + Cs, 2) channel sums of cat (UP_CAT_SA_SUMS: what moments(cat) returns) or its per-sample
    (pairs, pairs per sample) for gn_apply_fwd (UP_CAT_GN_PAIRS)."""
    Ct, HW = C + Cs, H * scale * W * scale
    out, res, ws, nws = None, None, None, 0
    if stats == UP_CAT_SA_SUMS:
        out = res = torch.empty((B, Ct, 2), dtype=torch.float64, device=z.device)
        ws = _ws.get(_lib.vrnet_moments_workspace(B, HW, Ct), z.device)
        nws = ws.numel()
    elif stats == UP_CAT_GN_PAIRS:
        per = _lib.vrnet_up_cat_pairs(B, HW, Ct)
        out = torch.empty((B, per, 2), dtype=torch.float64, device=z.device)
        res = (out, per)
    _check(_lib.vrnet_bn_relu_upsample_cat_f32(ptr(z), ldz, ptr(A), ptr(Dc), ptr(S), ptr(skip), lds, ptr(cat), ldc, B, H, W, C, Cs,
                                               scale, int(up_first), int(interleave), stats, ptr(out), ptr(ws), nws, stream()),
           "bn_relu_upsample_cat")
    return res


def minmax(p, n, mm):
    ws = _ws.get(_lib.vrnet_reduce_workspace(), p.device)
    _check(_lib.vrnet_minmax_f32(ptr(p), n, ptr(mm), ptr(ws), ws.numel(), stream()), "minmax")


def enhance_mul(p, x, mm, out, n):
    _check(_lib.vrnet_enhance_mul_f32(ptr(p), ptr(x), ptr(mm), ptr(out), n, stream()), "enhance_mul")


def enhance_fwd(p, x, mm, out, n):
    """minmax + enhance_mul in two launches; mm receives (min, max)."""
    ws = _ws.get(_lib.vrnet_reduce_workspace(), p.device)
    _check(_lib.vrnet_enhance_fwd_f32(ptr(p), ptr(x), ptr(mm), ptr(out), n, ptr(ws), ws.numel(), stream()), "enhance_fwd")


def enhance_bwd(dt, x, p, mm, dx, dp, n, accumulate_dx=0):
    ws = _ws.get(_lib.vrnet_reduce_workspace(), p.device)
    _check(_lib.vrnet_enhance_bwd_f32(ptr(dt), ptr(x), ptr(p), ptr(mm), ptr(dx), ptr(dp), n, accumulate_dx, ptr(ws),
                                      ws.numel(), stream()), "enhance_bwd")


def sa_coef_fwd(mom, cw, cb, sw, sb, gnw, gnb, B, HW, C, G, Pq, Qq, Mn):
    _check(_lib.vrnet_sa_coef_fwd(ptr(mom), ptr(cw), ptr(cb), ptr(sw), ptr(sb), ptr(gnw), ptr(gnb), B, HW, C, G, ptr(Pq),
                                  ptr(Qq), ptr(Mn), stream()), "sa_coef_fwd")


def sa_apply(x, ldx, Pq, Qq, Mn, y, ldy, B, HW, C):
    _check(_lib.vrnet_sa_apply_f32(ptr(x), ldx, ptr(Pq), ptr(Qq), ptr(Mn), ptr(y), ldy, B, HW, C, stream()), "sa_apply")


def sa_cat_sums(x, ldx, Pq, Qq, Mn, r, ldr, cat, ldc, B, HW, C):
    """ShuffleAttention apply + cat with r + 2-group shuffle -> cat, and the (B, 2C, 2) channel sums of cat (for the ECA gate)."""
    mom = torch.empty((B, 2 * C, 2), dtype=torch.float64, device=x.device)
    ws = _ws.get(_lib.vrnet_moments_workspace(B, HW, 2 * C), x.device)
    _check(_lib.vrnet_sa_cat_sums_f32(ptr(x), ldx, ptr(Pq), ptr(Qq), ptr(Mn), ptr(r), ldr, ptr(cat), ldc, B, HW, C, ptr(mom), ptr(ws),
                                      ws.numel(), stream()), "sa_cat_sums")
    return mom


def sa_bwd(dy, lddy, x, ldx, Pq, Qq, Mn, mom, params, dx, lddx, grads, EF, B, HW, C, G, accumulate_dx,
           accumulate_params):
    ws = _ws.get(_lib.vrnet_sa_bwd_workspace(B, HW, C), x.device)
    _check(_lib.vrnet_sa_bwd_f32(ptr(dy), lddy, ptr(x), ldx, ptr(Pq), ptr(Qq), ptr(Mn), ptr(mom),
                                 *[ptr(t) for t in params],
                                 ptr(dx), lddx, *[ptr(t) for t in grads], ptr(EF), B, HW, C, G, accumulate_dx,
                                 accumulate_params, ptr(ws), ws.numel(), stream()), "sa_bwd")


# ---- multi-tensor updates (optimizer step, EMA): tables are int64/int32/float32 device tensors built by optim.py
def mt_sgd(addrs, sizes, chunk_tensor, chunk_index, weight_decay, n_tensors, n_chunks, chunk_elems, lr, momentum, nesterov,
           first_step):
    _check(_lib.vrnet_mt_sgd_f32(ptr(addrs), ptr(sizes), ptr(chunk_tensor), ptr(chunk_index), ptr(weight_decay), n_tensors,
                                 n_chunks, chunk_elems, lr, momentum, int(nesterov), int(first_step), stream()), "mt_sgd")


def mt_adam(addrs, sizes, chunk_tensor, chunk_index, weight_decay, n_tensors, n_chunks, chunk_elems, lr, beta1, beta2, eps,
            step):
    _check(_lib.vrnet_mt_adam_f32(ptr(addrs), ptr(sizes), ptr(chunk_tensor), ptr(chunk_index), ptr(weight_decay), n_tensors,
                                  n_chunks, chunk_elems, lr, beta1, beta2, eps, step, stream()), "mt_adam")


def mt_ema(addrs, sizes, chunk_tensor, chunk_index, n_tensors, n_chunks, chunk_elems, decay):
    _check(_lib.vrnet_mt_ema_f32(ptr(addrs), ptr(sizes), ptr(chunk_tensor), ptr(chunk_index), n_tensors, n_chunks,
                                 chunk_elems, decay, stream()), "mt_ema")


class StepScalars(ctypes.Structure):
    """vrnet_step_scalars (include/vrnet_hip.h): the 16-byte record the `_dev` updates read from device memory."""
    _fields_ = [("lr", F), ("ema_decay", F), ("adam_bc1", F), ("adam_bc2_sqrt", F)]


def _scalars(s, name):
    if s.dtype != torch.float32 or s.numel() != 4 or not s.is_contiguous():
        raise RuntimeError(f"{name}: the step-scalar record is a contiguous float32 GPU tensor of 4 elements "
                           "(lr, ema_decay, adam_bc1, adam_bc2_sqrt)")
    return ptr(s)


def mt_sgd_dev(addrs, sizes, chunk_tensor, chunk_index, weight_decay, n_tensors, n_chunks, chunk_elems, scalars, momentum,
               nesterov):
    """mt_sgd with lr read from the record `scalars` in device memory (vrnet_mt_sgd_dev_f32)."""
    _check(_lib.vrnet_mt_sgd_dev_f32(ptr(addrs), ptr(sizes), ptr(chunk_tensor), ptr(chunk_index), ptr(weight_decay),
                                     n_tensors, n_chunks, chunk_elems, _scalars(scalars, "mt_sgd_dev"), momentum,
                                     int(nesterov), stream()), "mt_sgd_dev")


def mt_adam_dev(addrs, sizes, chunk_tensor, chunk_index, weight_decay, n_tensors, n_chunks, chunk_elems, scalars, beta1,
                beta2, eps):
    """mt_adam with lr and the bias corrections read from the record (vrnet_mt_adam_dev_f32)."""
    _check(_lib.vrnet_mt_adam_dev_f32(ptr(addrs), ptr(sizes), ptr(chunk_tensor), ptr(chunk_index), ptr(weight_decay),
                                      n_tensors, n_chunks, chunk_elems, _scalars(scalars, "mt_adam_dev"), beta1, beta2, eps,
                                      stream()), "mt_adam_dev")


def mt_ema_dev(addrs, sizes, chunk_tensor, chunk_index, n_tensors, n_chunks, chunk_elems, scalars):
    """mt_ema with the decay read from the record (vrnet_mt_ema_dev_f32)."""
    _check(_lib.vrnet_mt_ema_dev_f32(ptr(addrs), ptr(sizes), ptr(chunk_tensor), ptr(chunk_index), n_tensors, n_chunks,
                                     chunk_elems, _scalars(scalars, "mt_ema_dev"), stream()), "mt_ema_dev")


def adam_bias_correction(beta1, beta2, step):
    """(bc1, bc2_sqrt) as vrnet_mt_adam_f32 derives them from `step`: C's double-precision pow / sqrt, rounded to float
    (host only, no GPU needed)."""
    bc1, bc2 = F(), F()
    _check(_lib.vrnet_adam_bias_correction(float(beta1), float(beta2), int(step), ctypes.byref(bc1), ctypes.byref(bc2)),
           "adam_bias_correction")
    return bc1.value, bc2.value


def mt_copy(addrs, sizes, chunk_tensor, chunk_index, n_tensors, n_chunks, chunk_elems):
    _check(_lib.vrnet_mt_copy_f32(ptr(addrs), ptr(sizes), ptr(chunk_tensor), ptr(chunk_index), n_tensors, n_chunks,
                                  chunk_elems, stream()), "mt_copy")


def decode_outputs(levels, input_h, input_w, out):
    """levels: list of contiguous (B, C, h, w) fp32 GPU tensors; out: (B, sum h*w, C)."""
    n = len(levels)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in levels])
    hs = (ctypes.c_int * n)(*[t.shape[2] for t in levels])
    ws = (ctypes.c_int * n)(*[t.shape[3] for t in levels])
    _check(_lib.vrnet_decode_outputs_f32(ptrs, hs, ws, n, levels[0].shape[0], levels[0].shape[1], float(input_h),
                                         float(input_w), ptr(out), stream()), "decode_outputs")


def detect_select(pred, num_classes, conf_thres, rows, scores, cls, ids, counts):
    """pred (B, A, C) fp32 -> the per-image candidate lists of non_max_suppression (vrnet_detect_select_f32)."""
    B, A, C = pred.shape
    _check(_lib.vrnet_detect_select_f32(ptr(pred), B, A, C, num_classes, float(conf_thres), ptr(rows), ptr(scores), ptr(cls),
                                        ptr(ids), ptr(counts), stream()), "detect_select")


def nms_workspace_bytes(segments, n_max):
    return _lib.vrnet_nms_workspace_bytes(segments, n_max)


def nms_segmented(rows, scores, classes, ids, counts, segments, stride, n_max, iou_thres, workspace, keep, kept,
                  rows_out=None):
    """Class-aware greedy NMS over `segments` segments (vrnet_nms_segmented_f32); rows (..., ld) holds the boxes in
    columns 0-3, ids / counts may be None."""
    _check(_lib.vrnet_nms_segmented_f32(ptr(rows), rows.shape[-1], ptr(scores), ptr(classes), ptr(ids), ptr(counts),
                                        segments, stride, n_max, float(iou_thres), ptr(workspace), workspace.numel(),
                                        ptr(keep), ptr(kept), ptr(rows_out), stream()), "nms_segmented")


def nms_capped(rows, scores, classes, ids, counts, segments, stride, cap, iou_thres, workspace, keep, kept, rows_out, flag):
    """nms_segmented with a fixed capacity (vrnet_nms_capped_f32): every candidate is ranked, ranks < cap enter the NMS;
    counts (segments) int32 is required, flag (1) int32 receives bit 8 when a segment has more candidates than cap."""
    _check(_lib.vrnet_nms_capped_f32(ptr(rows), rows.shape[-1], ptr(scores), ptr(classes), ptr(ids), ptr(counts), segments,
                                     stride, cap, float(iou_thres), ptr(workspace), workspace.numel(), ptr(keep), ptr(kept),
                                     ptr(rows_out), ptr(flag), stream()), "nms_capped")


def detect_finish(rows, kept, num_classes, image_shape, offset, scale, rows_out, draw_rows, offsets, det_counts, flag, geom=None,
                  capacity=None, fn="detect_finish"):
    """The kept rows (B, cap, 7) of nms_capped -> rows in pixels of the original image, the renderer's box rows with
    their offsets and the class counts (vrnet_detect_finish_f32).  offset / scale: the (y, x) float64 pairs of
    yolo_correct_boxes; image_shape = (ih, iw).  With geom (`_table_call`) all three are None: the shape and the un-map
    scalars of image b come from geom[b], and capacity = (ihm, iwm) (vrnet_detect_finish_ragged_f32)."""
    table = _table_call(fn, geom, (("image_shape", image_shape, None), ("offset", offset, None), ("scale", scale, None)),
                       (("capacity", capacity, None),))
    B, cap = rows.shape[:2]
    _tensors(fn, ((rows, (B, cap, 7), torch.float32), (kept, (B,), torch.int32), (rows_out, (B, cap, 7), torch.float32),
                  (draw_rows, (B * cap, 5), torch.int32), (offsets, (B + 1,), torch.int32),
                  (det_counts, (B, num_classes), torch.int64), (flag, (1,), torch.int32)))
    outs = (rows_out, draw_rows, offsets, det_counts, flag)
    if table:
        _check(_lib.vrnet_detect_finish_ragged_f32(ptr(rows), ptr(kept), _geom(geom, B, fn), B, cap, int(num_classes), int(capacity[0]),
                                                   int(capacity[1]), *map(ptr, outs), stream()), fn)
    else:
        _check(_lib.vrnet_detect_finish_f32(ptr(rows), ptr(kept), B, cap, int(num_classes), int(image_shape[0]), int(image_shape[1]),
                                            float(offset[0]), float(offset[1]), float(scale[0]), float(scale[1]), *map(ptr, outs),
                                            stream()), fn)


def eval_append(rows, kept, gt, gt_count, cursor, arena, flag):
    """One batch of kept rows and ground truths -> the record arena of a validation pass, at the image slots cursor ..
    cursor + B - 1 (vrnet_eval_append_f32).  rows (B, cap, 7) / kept (B): `detect_finish`'s rows_out / kept; gt (B, max_gt, 5)
    int32 with gt_count (B); cursor (1) int32; arena: a dict of det_label (N, max_boxes) int32, det_score (N, max_boxes)
    float64, det_box (N, max_boxes, 4) float64, det_count (N) int32, gt_label (N, max_gt) int32, gt_box (N, max_gt, 4)
    float64, gt_n (N) int32; flag (1) int32 receives bits 32 (no room: nothing written), 64 (gt_count > max_gt), 128 (a
    value int() cannot take)."""
    B, cap = rows.shape[:2]
    max_gt = gt.shape[1] if gt.dim() == 3 else -1
    N, max_boxes = arena["det_label"].shape if arena["det_label"].dim() == 2 else (-1, -1)
    i32, f64 = torch.int32, torch.float64
    for name, t, sh, dt in (("rows", rows, (B, cap, 7), torch.float32), ("kept", kept, (B,), i32), ("gt", gt, (B, max_gt, 5), i32),
                            ("gt_count", gt_count, (B,), i32), ("cursor", cursor, (1,), i32), ("flag", flag, (1,), i32),
                            ("det_label", arena["det_label"], (N, max_boxes), i32),
                            ("det_score", arena["det_score"], (N, max_boxes), f64),
                            ("det_box", arena["det_box"], (N, max_boxes, 4), f64), ("det_count", arena["det_count"], (N,), i32),
                            ("gt_label", arena["gt_label"], (N, max_gt), i32), ("gt_box", arena["gt_box"], (N, max_gt, 4), f64),
                            ("gt_n", arena["gt_n"], (N,), i32)):
        if tuple(t.shape) != sh or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"eval_append: {name} must be a contiguous {dt} GPU tensor of shape {sh}, got {t.dtype} "
                               f"{tuple(t.shape)}")
    _check(_lib.vrnet_eval_append_f32(ptr(rows), ptr(kept), B, cap, ptr(gt), ptr(gt_count), max_gt, ptr(cursor), N, max_boxes,
                                      ptr(arena["det_label"]), ptr(arena["det_score"]), ptr(arena["det_box"]),
                                      ptr(arena["det_count"]), ptr(arena["gt_label"]), ptr(arena["gt_box"]), ptr(arena["gt_n"]),
                                      ptr(flag), stream()), "eval_append")


def radar_normalise(radar, out, normalise=True, ws=None):
    """radar (B, ...) float32 / float64 -> out, the same shape in float32: each frame min-max normalised as
    preprocess_input_radar does it, or (normalise=False) cast (vrnet_radar_normalise)."""
    if radar.dtype not in (torch.float32, torch.float64) or not radar.is_contiguous() or radar.dim() < 2 or radar.numel() == 0:
        raise RuntimeError(f"radar_normalise: expected contiguous float32 / float64 maps (B, ...), got {radar.dtype} {tuple(radar.shape)}")
    if out.dtype != torch.float32 or out.shape != radar.shape or not out.is_contiguous():
        raise RuntimeError(f"radar_normalise: out must be a contiguous float32 tensor of shape {tuple(radar.shape)}")
    B = radar.shape[0]
    if normalise and ws is None:
        ws = torch.empty(_lib.vrnet_radar_workspace_bytes(B) // 8, dtype=torch.float64, device=radar.device)
    _check(_lib.vrnet_radar_normalise(ptr(radar), int(radar.dtype == torch.float64), B, radar.numel() // B, int(bool(normalise)),
                                      ptr(out), ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(), stream()),
           "radar_normalise")


def batch_formats(img_u8, png_u8, num_classes_seg, images=None, png_out=None, onehot=None):
    """Letterboxed batch as bytes -> the tensors the reference's collate function ships (vrnet_batch_formats_u8):
    img_u8 (B,H,W,3) uint8 -> images (B,3,H,W) f32; png_u8 (B,H,W) uint8 -> png (B,H,W) int64, onehot (B,H,W,ns+1) f32."""
    src = img_u8 if img_u8 is not None else png_u8
    B, H, W = src.shape[:3]
    _tensors("batch_formats", ((img_u8, (B, H, W, 3), torch.uint8), (png_u8, (B, H, W), torch.uint8)))
    if img_u8 is not None and images is None:
        images = torch.empty((B, 3, H, W), dtype=torch.float32, device=src.device)
    if png_u8 is not None:
        if png_out is None:
            png_out = torch.empty((B, H, W), dtype=torch.int64, device=src.device)
        if onehot is None:
            onehot = torch.empty((B, H, W, num_classes_seg + 1), dtype=torch.float32, device=src.device)
    _check(_lib.vrnet_batch_formats_u8(ptr(img_u8), ptr(png_u8), B, H, W, int(num_classes_seg), ptr(images), ptr(png_out),
                                       ptr(onehot), stream()), "batch_formats")
    return images, png_out, onehot


def letterbox_workspace_bytes(B, ih, iw, nh, nw):
    return _lib.vrnet_letterbox_workspace(B, ih, iw, nh, nw)


def letterbox(img_u8, label_u8, H, W, nw=None, nh=None, dx=None, dy=None, canvas=None, images=None, label_out=None, ws=None,
              geom=None, max_taps=None, flag=None, fn="letterbox"):
    """Raw frames -> the letterboxed batch, Pillow's bytes (vrnet_letterbox_u8): img_u8 (B,ih,iw,3) uint8 RGB, label_u8
    (B,ih,iw) uint8 or None; the window nw x nh at column dx, row dy of the W x H canvas.  Outputs (None = not wanted):
    canvas (B,H,W,3) uint8, images (B,3,H,W) f32 normalised as batch_formats does, label_out (B,H,W) uint8.  ws: a uint8
    tensor of letterbox_workspace_bytes(B, ih, iw, nh, nw) bytes (default: this stream's scratch arena).  With geom
    (`_table_call`) the inputs are padded slots (B,ihm,iwm,..), the window of image b comes from geom[b] in place of nw, nh, dx,
    dy, max_taps is the tap capacity of a table entry and ws has letterbox_ragged_workspace_bytes (vrnet_letterbox_ragged_u8)."""
    table = _table_call(fn, geom, (("nw", nw, None), ("nh", nh, None), ("dx", dx, None), ("dy", dy, None)),
                       (("max_taps", max_taps, None),))
    m = "m" if table else ""
    src = img_u8 if img_u8 is not None else label_u8
    if src is None or src.dim() < 3:
        raise RuntimeError(f"{fn}: expected frames (B, ih{m}, iw{m}, 3) and / or label maps (B, ih{m}, iw{m})")
    B, ih, iw = src.shape[:3]
    _tensors(fn, ((img_u8, (B, ih, iw, 3), torch.uint8), (label_u8, (B, ih, iw), torch.uint8), (canvas, (B, H, W, 3), torch.uint8),
                  (images, (B, 3, H, W), torch.float32), (label_out, (B, H, W), torch.uint8), (flag, (1,), torch.int32)))
    # a table call asks for its size even when the caller brings a workspace
    need = _lib.vrnet_letterbox_ragged_workspace(B, ih, iw, int(H), int(W), int(max_taps)) if table else None
    if ws is None:
        ws = _ws.get(need if table else _lib.vrnet_letterbox_workspace(B, ih, iw, nh, nw), src.device)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise RuntimeError(f"{fn}: the workspace must be a contiguous uint8 tensor, got {ws.dtype}")
    if table:
        _check(_lib.vrnet_letterbox_ragged_u8(ptr(img_u8), ptr(label_u8), _geom(geom, B, fn), B, ih, iw, int(H), int(W), int(max_taps),
                                              ptr(canvas), ptr(images), ptr(label_out), ptr(flag), ptr(ws), ws.numel(), stream()), fn)
    else:
        _check(_lib.vrnet_letterbox_u8(ptr(img_u8), ptr(label_u8), B, ih, iw, int(H), int(W), int(nw), int(nh), int(dx), int(dy),
                                       ptr(canvas), ptr(images), ptr(label_out), ptr(ws), ws.numel(), stream()), fn)


def render(frames, class_map, out, palette=None, mix_type=0, alpha=0.7, boxes=None, box_offsets=None, box_palette=None,
           thickness=1, counts=None, flag=None, geom=None, fn="render"):
    """The rendered frames (vrnet_render_u8): frames / out (B,ih,iw,3) uint8, class_map (B,ih,iw) uint8 or None, palette
    (n,3) uint8, boxes (N,5) int32 with box_offsets (B+1) int32 and box_palette (m,3) uint8, counts (B,n) int64 (overwritten;
    n = counts.shape[1] when there is no palette), flag (1) int32 (data-error bits, OR-ed in).  out may be frames when there
    is no class map.  With geom (`_table_call`) frames / out / class_map are padded slots, ih, iw and the thickness of image b
    come from geom[b] and out must not be the frames (vrnet_render_ragged_u8)."""
    table = _table_call(fn, geom, (("thickness", thickness, 1),))
    m = "m" if table else ""
    if frames is None or frames.dim() != 4 or frames.shape[-1] != 3 or \
            not (table or (frames.dtype == torch.uint8 and frames.is_contiguous())):
        raise RuntimeError(f"{fn}: expected contiguous uint8 frames of shape (B, ih{m}, iw{m}, 3)")
    B, ih, iw = frames.shape[:3]
    n_colors = palette.shape[0] if palette is not None else (counts.shape[1] if counts is not None else 0)
    n_rows = 0 if boxes is None else boxes.shape[0]
    n_box_colors = 0 if box_palette is None else box_palette.shape[0]
    _tensors(fn, (
        (frames, (B, ih, iw, 3), torch.uint8), (out, (B, ih, iw, 3), torch.uint8), (class_map, (B, ih, iw), torch.uint8),
        (palette, (n_colors, 3), torch.uint8), (boxes, (n_rows, 5), torch.int32), (box_offsets, (B + 1,), torch.int32),
        (counts, (B, n_colors), torch.int64), (flag, (1,), torch.int32), (box_palette, (n_box_colors, 3), torch.uint8)))
    if out is None or (n_rows and (box_offsets is None or box_palette is None)):
        raise RuntimeError(f"{fn}: out is required, and box rows need box_offsets and a box_palette")
    picture = (ptr(palette), n_colors, int(mix_type), float(alpha), ptr(boxes) if n_rows else None, ptr(box_offsets), n_rows,
               ptr(box_palette), n_box_colors)
    if table:
        _check(_lib.vrnet_render_ragged_u8(ptr(frames), ptr(class_map), _geom(geom, B, fn), B, ih, iw, *picture, ptr(out),
                                           ptr(counts), ptr(flag), stream()), fn)
    else:
        _check(_lib.vrnet_render_u8(ptr(frames), ptr(class_map), B, ih, iw, *picture, int(thickness), ptr(out), ptr(counts),
                                    ptr(flag), stream()), fn)


def _heat_levels(fn, levels, H, W):
    """The three raw detection maps of an (H, W) input: (B, 5 + nc, H/8, W/8), (.., H/16, W/16), (.., H/32, W/32) fp32."""
    if len(levels) != 3 or levels[0] is None or levels[0].dim() != 4 or levels[0].shape[1] < 6:
        raise RuntimeError(f"{fn}: expected three detection maps (B, 5 + nc, h, w) with nc >= 1")
    B, C = levels[0].shape[:2]
    _tensors(fn, tuple((t, (B, C, H // s, W // s), torch.float32) for t, s in zip(levels, (8, 16, 32))))
    return B, C - 5


def heatmap_workspace_bytes(B, H, W):
    return _lib.vrnet_heatmap_workspace(B, H, W)


def heatmap(levels, H, W, mask, minmax, ws, window=0, dx=0, dy=0, nw=0, nh=0, frames=None, cmap=None, alpha=0.5, out=None,
            geom=None, flag=None, fn="heatmap"):
    """yolo.py:288-351 on the device (vrnet_heatmap_f32): levels the three raw detection maps of an (H, W) input -> mask
    (B, ih, iw) uint8 and minmax (B, 2) int32; with out (B, ih, iw, 3) uint8 also the blend of cmap (256, 3) uint8 over
    frames (B, ih, iw, 3) uint8.  window = 1 maps the pixels through the letterbox window (dx, dy, nw, nh).  ws:
    heatmap_workspace_bytes(B, H, W) bytes.  With geom (`_table_call`) mask, frames and out are padded slots, ih, iw and the
    window of image b come from geom[b], 0 outside the image, and ws has heatmap_ragged_workspace_bytes
    (vrnet_heatmap_ragged_f32)."""
    table = _table_call(fn, geom, (("dx", dx, 0), ("dy", dy, 0), ("nw", nw, 0), ("nh", nh, 0)))
    m = "m" if table else ""
    B, nc = _heat_levels(fn, levels, int(H), int(W))
    if mask is None or mask.dim() != 3:
        raise RuntimeError(f"{fn}: mask (B, ih{m}, iw{m}) is required")
    ih, iw = mask.shape[1:]
    _tensors(fn, ((mask, (B, ih, iw), torch.uint8), (minmax, (B, 2), torch.int32), (frames, (B, ih, iw, 3), torch.uint8),
                  (out, (B, ih, iw, 3), torch.uint8), (cmap, (256, 3), torch.uint8), (flag, (1,), torch.int32)))
    lv, picture = [ptr(t) for t in levels], (ptr(frames), ptr(cmap), float(alpha), ptr(mask), ptr(out), ptr(minmax))
    if table:
        _check(_lib.vrnet_heatmap_ragged_f32(*lv, _geom(geom, B, fn), B, nc, int(H), int(W), ih, iw, int(window), *picture, ptr(flag),
                                             ptr(ws), ws.numel(), stream()), fn)
    else:
        _check(_lib.vrnet_heatmap_f32(*lv, B, nc, int(H), int(W), ih, iw, int(window), int(dx), int(dy), int(nw), int(nh), *picture,
                                      ptr(ws), ws.numel(), stream()), fn)


def yolo_loss(levels, grads, strides, labels, counts, max_gt, grad_scale, out, fg=None, matched=None, piou=None):
    """levels / grads: lists of contiguous (B, C, h, w) fp32 GPU tensors (grads None = value only)."""
    n = len(levels)
    B, C = levels[0].shape[:2]
    A = sum(t.shape[2] * t.shape[3] for t in levels)
    lv = (ctypes.c_void_p * n)(*[t.data_ptr() for t in levels])
    gr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads]) if grads is not None else None
    hs = (ctypes.c_int * n)(*[t.shape[2] for t in levels])
    ws_ = (ctypes.c_int * n)(*[t.shape[3] for t in levels])
    st = (ctypes.c_float * n)(*[float(s) for s in strides])
    ws = _ws.get(_lib.vrnet_yolo_loss_workspace(B, A, max_gt, C - 5), levels[0].device)
    _check(_lib.vrnet_yolo_loss_f32(lv, gr, hs, ws_, st, n, B, C, ptr(labels), ptr(counts), max_gt, float(grad_scale),
                                    ptr(out), ptr(fg), ptr(matched), ptr(piou), ptr(ws), ws.numel(), stream()), "yolo_loss")


def seg_loss(x, png, onehot, weights, focal, dice, alpha, gamma, beta, smooth, grad_scale, out, dx):
    B, C, H, W = x.shape
    ws = _ws.get(_lib.vrnet_seg_loss_workspace(B, C, H * W), x.device)
    _check(_lib.vrnet_seg_loss_f32(ptr(x), ptr(png), ptr(onehot), ptr(weights), B, C, H * W, int(focal), int(bool(dice)),
                                   float(alpha), float(gamma), float(beta), float(smooth), float(grad_scale), ptr(out),
                                   ptr(dx), ptr(ws), ws.numel(), stream()), "seg_loss")


def seg_fscore(x, onehot, beta, smooth, threshold, out, counts=None):
    """x (B, C, H, W) fp32, onehot (B, H, W, C+1) fp32 -> out[0] = f_score (vrnet_seg_fscore_f32); counts (3C) fp64, if
    given, receives the totals tp[C], sp[C], st[C]."""
    B, C, H, W = x.shape
    ws = _ws.get(_lib.vrnet_seg_loss_workspace(B, C, H * W), x.device)
    _check(_lib.vrnet_seg_fscore_f32(ptr(x), ptr(onehot), B, C, H * W, float(beta), float(smooth), float(threshold),
                                     ptr(out), ptr(counts), ptr(ws), ws.numel(), stream()), "seg_fscore")


def seg_predict_workspace_bytes(B, C, nh, nw):
    return _lib.vrnet_seg_predict_workspace(B, C, nh, nw)


def seg_predict(x, top, left, nh, nw, out, ws, geom=None, flag=None, fn="seg_predict"):
    """x (B, C, H, W) fp32 -> out (B, oh, ow) uint8: arg-max of the bilinear resize of the window's softmax
    (vrnet_seg_predict_f32); ws: seg_predict_workspace_bytes(B, C, nh, nw) bytes.  With geom (`_table_call`) top, left, nh and
    nw are None: out is (B, ihm, iwm), the window and size of image b come from geom[b], 0 outside the image, and ws has
    seg_predict_ragged_workspace_bytes(B, C, H, W) bytes (vrnet_seg_predict_ragged_f32)."""
    B, C, H, W = x.shape
    if _table_call(fn, geom, (("top", top, None), ("left", left, None), ("nh", nh, None), ("nw", nw, None))):
        _tensors(fn, ((x, (B, C, H, W), torch.float32), (out, (B,) + tuple(out.shape[1:3]), torch.uint8), (flag, (1,), torch.int32)))
        _check(_lib.vrnet_seg_predict_ragged_f32(ptr(x), _geom(geom, B, fn), B, C, H, W, out.shape[1], out.shape[2], ptr(out),
                                                 ptr(flag), ptr(ws), ws.numel(), stream()), fn)
    else:
        _check(_lib.vrnet_seg_predict_f32(ptr(x), B, C, H, W, top, left, nh, nw, out.shape[1], out.shape[2], ptr(out), ptr(ws),
                                          ws.numel(), stream()), fn)


def confusion_hist(label, pred, n, hist):
    """hist (n, n) int64 += counts of (label, pred) pairs with both in [0, n) (vrnet_confusion_hist); label / pred are
    contiguous uint8 or int64 tensors of one size."""
    _check(_lib.vrnet_confusion_hist(ptr(label), label.element_size(), ptr(pred), pred.element_size(), label.numel(), n,
                                     ptr(hist), stream()), "confusion_hist")


def det_map(det_image, det_label, det_score, det_box, order, det_offsets, gt_box, gt_difficult, gt_perm, gt_offsets,
            n_images, num_classes, min_overlap, score_threhold, out, ws=None):
    """VOC AP matching and curves for len(min_overlap) IoU thresholds (vrnet_det_map_f64, which documents every array).
    out: dict of the output tensors by the header's names; out["rec"] / out["prec"] may be None."""
    D, G, T = det_score.numel(), gt_difficult.numel(), len(min_overlap)
    if ws is None:
        ws = _ws.get(_lib.vrnet_det_map_workspace_bytes(D, G, T), det_offsets.device)
    thr = (ctypes.c_double * T)(*[float(v) for v in min_overlap])
    _check(_lib.vrnet_det_map_f64(ptr(det_image), ptr(det_label), ptr(det_score), ptr(det_box), ptr(order), ptr(det_offsets), D,
                                  ptr(gt_box), ptr(gt_difficult), ptr(gt_perm), ptr(gt_offsets), G, int(n_images),
                                  int(num_classes), thr, T, float(score_threhold),
                                  *[ptr(out[k]) for k in ("match", "ovmax", "tp", "fp", "rec", "prec", "n_gt", "n_img", "n_tp",
                                                          "ap", "f1", "recall", "precision", "lamr", "map")],
                                  ptr(ws), ws.numel(), stream()), "det_map")


def coco_map(det_box, order, rank, class_slot, det_offsets, group_start, group_gt, group_ws, lds_bytes, slice_bytes, gt_box,
             gt_area, gt_crowd, gt_label, gt_perm, num_classes, zero_id_gt, iou_thrs, rec_thrs, out, ws=None):
    """COCO bbox evaluation (vrnet_coco_map_f64, which documents every array).  out: dict of the output tensors by the
    header's names."""
    D, G, NG = rank.numel(), gt_label.numel(), group_ws.numel()
    if ws is None:
        ws = _ws.get(_lib.vrnet_coco_map_workspace_bytes(D, int(slice_bytes)), det_offsets.device)
    _check(_lib.vrnet_coco_map_f64(ptr(det_box), ptr(order), ptr(rank), ptr(class_slot), ptr(det_offsets), D, ptr(group_start),
                                   ptr(group_gt), ptr(group_ws), NG, int(lds_bytes), int(slice_bytes), ptr(gt_box),
                                   ptr(gt_area), ptr(gt_crowd), ptr(gt_label), ptr(gt_perm), G, int(num_classes),
                                   int(zero_id_gt), ptr(iou_thrs), ptr(rec_thrs),
                                   *[ptr(out[k]) for k in ("dt_match", "dt_code", "n_gt", "precision", "recall", "stats")],
                                   ptr(ws), ws.numel(), stream()), "coco_map")


def mean_square(tensors):
    """loss = sum_k mean(t_k^2) (a 1-element fp32 tensor) over contiguous fp32 tensors: two launches."""
    k = len(tensors)
    PA, LA = ctypes.c_void_p * k, ctypes.c_long * k
    n = LA(*[t.numel() for t in tensors])
    ws = _ws.get(_lib.vrnet_mean_square_workspace(k, n), tensors[0].device)
    loss = torch.empty((1,), dtype=torch.float32, device=tensors[0].device)
    _check(_lib.vrnet_mean_square_f32(k, PA(*[ptr(t) for t in tensors]), n, ptr(loss), ptr(ws), ws.numel(), stream()), "mean_square")
    return loss


def mean_square_bwd(tensors, g, grads):
    """grads[k] = (2 g / n_k) tensors[k]; g: 1-element device tensor."""
    k = len(tensors)
    PA, LA = ctypes.c_void_p * k, ctypes.c_long * k
    _check(_lib.vrnet_mean_square_bwd_f32(k, PA(*[ptr(t) for t in tensors]), LA(*[t.numel() for t in tensors]), ptr(g),
                                          PA(*[ptr(t) for t in grads]), stream()), "mean_square_bwd")


# ---- fused passes of the fusion blocks (csrc/fusion.hip)
def fusion_chunks(n, C):
    """Workgroups / partial entries of the fused fusion-block kernels for a contiguous tensor (0: shape not supported)."""
    return _lib.vrnet_fusion_chunks(n, C)


def fusion_fold_chunks(n, C):
    """Entries of the (min, max) / four-sum partials (bn_relu_minmax, bn_bwd_enhance)."""
    return _lib.vrnet_fusion_fold_chunks(n, C)


def bn_relu_minmax(z, A, D, S, p, n, C, mmpart):
    _check(_lib.vrnet_bn_relu_minmax_f32(ptr(z), ptr(A), ptr(D), ptr(S), ptr(p), n, C, ptr(mmpart), stream()), "bn_relu_minmax")


def bn_relu_res_stats(z, A, D, S, res, s, n, C, colpart):
    _check(_lib.vrnet_bn_relu_res_stats_f32(ptr(z), ptr(A), ptr(D), ptr(S), ptr(res), ptr(s), n, C, ptr(colpart), stream()),
           "bn_relu_res_stats")


def enhance_stats(p, x, mmpart, nmm, mm, t, n, C, colpart):
    _check(_lib.vrnet_enhance_stats_f32(ptr(p), ptr(x), ptr(mmpart), nmm, ptr(mm), ptr(t), n, C, ptr(colpart), stream()),
           "enhance_stats")


def bn_bwd_enhance(g, t, A, E, D, S, x, p, mm, dt, n, C, sums4):
    _check(_lib.vrnet_bn_bwd_enhance_f32(ptr(g), ptr(t), ptr(A), ptr(E), ptr(D), ptr(S), ptr(x), ptr(p), ptr(mm), ptr(dt), n, C,
                                         ptr(sums4), stream()), "bn_bwd_enhance")


def enhance_bwd_stats(dt, x, p, mm, sums4, nsums, z, fA, fD, fS, dx, dp, n, C, accumulate_dx, colpart):
    _check(_lib.vrnet_enhance_bwd_stats_f32(ptr(dt), ptr(x), ptr(p), ptr(mm), ptr(sums4), nsums, ptr(z), ptr(fA), ptr(fD), ptr(fS),
                                            ptr(dx), ptr(dp), n, C, accumulate_dx, ptr(colpart), stream()), "enhance_bwd_stats")


def bn_bwd_next_stats(g, s, A, E, D, S, z, fwd, ds, n, C, colpart):
    _check(_lib.vrnet_bn_bwd_next_stats_f32(ptr(g), ptr(s), ptr(A), ptr(E), ptr(D), ptr(S), ptr(z), ptr(fwd[0]), ptr(fwd[1]),
                                            ptr(fwd[2]), ptr(ds), n, C, ptr(colpart), stream()), "bn_bwd_next_stats")


def bn_coef_fwd_from_chunks(partial, nchunks, count, gamma, beta, eps, momentum, rmean, rvar, nbt, C, A, Dc, S, mean_rstd):
    _check(_lib.vrnet_bn_coef_fwd_from_chunks(ptr(partial), nchunks, count, ptr(gamma), ptr(beta), eps, momentum, ptr(rmean), ptr(rvar),
                                              ptr(nbt), C, ptr(A), ptr(Dc), ptr(S), ptr(mean_rstd), stream()), "bn_coef_fwd_from_chunks")


def bn_coef_bwd_from_chunks(partial, nchunks, count, mean_rstd, gamma, training, C, A, E, Dc, S, dgamma, dbeta, accumulate):
    _check(_lib.vrnet_bn_coef_bwd_from_chunks(ptr(partial), nchunks, count, ptr(mean_rstd), ptr(gamma), 1 if training else 0, C, ptr(A),
                                              ptr(E), ptr(Dc), ptr(S), ptr(dgamma), ptr(dbeta), accumulate, stream()),
           "bn_coef_bwd_from_chunks")


# ---- ragged batches (include/vrnet_hip.h "ragged batches"): per-image geometry from a device table -------------------
GEOM_BYTES = 80          # sizeof(vrnet_frame_geom)
FLAG_GEOMETRY = 256      # VR_FLAG_GEOMETRY of csrc/common.h
FLAG_BOX_COUNT = 512     # VR_FLAG_BOX_COUNT of csrc/common.h: box_targets_ragged clamped a count outside [0, max_gt]


AUG_BYTES = 816          # sizeof(vrnet_aug_rec)
AUG_POST_BYTES = 112     # sizeof(vrnet_aug_post_rec)
MOSAIC_BYTES = 976       # sizeof(vrnet_mosaic_rec)


class _TableKind:
    """One kind of per-image device table: `what` it is called in messages, its record bytes, the wrapper names it gives
    ("{}_ragged", "augment_{}", "mosaic_{}" -- the C entry points are vrnet_<name>_<type>), the workspace function of its
    frames call, and `sources`: the table has one record per OUTPUT image over S source slots, so the batch size comes from
    the table and the C calls take S in front of it (Mosaic).  Otherwise there is one record per input."""

    def __init__(self, what, nbytes, name, workspace, sources=False):
        self.what, self.nbytes, self.name, self.workspace, self.sources = what, nbytes, name, workspace, sources
        self.n = "S" if sources else "B"                  # the inputs' leading dimension, in messages


_GEOM = _TableKind("geometry", GEOM_BYTES, "{}_ragged", "vrnet_letterbox_ragged_workspace")
_AUG = _TableKind("augmentation", AUG_BYTES, "augment_{}", "vrnet_letterbox_ragged_workspace")
_AUG_POST = _TableKind("post", AUG_POST_BYTES, "augment_post_{}", None)
_MOSAIC = _TableKind("Mosaic", MOSAIC_BYTES, "mosaic_{}", "vrnet_mosaic_workspace_bytes", sources=True)


def _table(kind, t, n_in, fn):
    """The table: a contiguous uint8 GPU tensor (B, kind.nbytes), 8-byte aligned (`data.frame_geometry`, `data.augment_bytes`
    and `data.mosaic_bytes` pack them); B is n_in, the inputs' count, unless the kind has sources.  Returns the leading
    arguments of the C call after the inputs: (table, B), or (S, table, B)."""
    if t is None or t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != kind.nbytes or not (kind.sources or t.shape[0] == n_in) or \
            not t.is_contiguous() or not t.is_cuda or t.data_ptr() % 8:
        raise RuntimeError(f"{fn}: the {kind.what} table must be a contiguous, 8-byte aligned uint8 GPU tensor of shape "
                           f"({'B' if kind.sources else n_in}, {kind.nbytes})")
    return (n_in, ptr(t), t.shape[0]) if kind.sources else (ptr(t), n_in)


def _geom(geom, B, fn):
    return _table(_GEOM, geom, B, fn)[0]


# the `_ragged` names of the inference-side frame ops: each is the fixed-name body with the table (`_table_call`)
def letterbox_ragged(img_u8, label_u8, geom, H, W, max_taps, canvas=None, images=None, label_out=None, flag=None, ws=None):
    letterbox(img_u8, label_u8, H, W, None, None, None, None, canvas, images, label_out, ws, geom, max_taps, flag, "letterbox_ragged")


def detect_finish_ragged(rows, kept, geom, num_classes, capacity, rows_out, draw_rows, offsets, det_counts, flag):
    detect_finish(rows, kept, num_classes, None, None, None, rows_out, draw_rows, offsets, det_counts, flag, geom, capacity,
                  "detect_finish_ragged")


def seg_predict_ragged(x, geom, out, ws, flag=None):
    seg_predict(x, None, None, None, None, out, ws, geom, flag, "seg_predict_ragged")


def render_ragged(frames, class_map, geom, out, palette=None, mix_type=0, alpha=0.7, boxes=None, box_offsets=None,
                  box_palette=None, counts=None, flag=None):
    render(frames, class_map, out, palette, mix_type, alpha, boxes, box_offsets, box_palette, 1, counts, flag, geom, "render_ragged")


def heatmap_ragged(levels, geom, H, W, mask, minmax, ws, window=1, frames=None, cmap=None, alpha=0.5, out=None, flag=None):
    heatmap(levels, H, W, mask, minmax, ws, window, 0, 0, 0, 0, frames, cmap, alpha, out, geom, flag, "heatmap_ragged")


def letterbox_ragged_workspace_bytes(B, ihm, iwm, H, W, max_taps):
    return _lib.vrnet_letterbox_ragged_workspace(B, ihm, iwm, H, W, max_taps)


def seg_predict_ragged_workspace_bytes(B, C, H, W):
    return _lib.vrnet_seg_predict_ragged_workspace(B, C, H, W)


# ---- the frame modes of training: the plain letterbox, the augmentation and the Mosaic run the same four operations ----
# under their own table kind; one body per operation, and the public wrappers below are one call each
def _seg_targets(kind, label_u8, tab, H, W, num_classes_seg, png_out, onehot, flag):
    fn = kind.name.format("seg_targets")
    if label_u8 is None or label_u8.dim() != 3:
        raise RuntimeError(f"{fn}: expected label maps ({kind.n}, ihm, iwm)")
    n, ihm, iwm = label_u8.shape
    H, W, ns = int(H), int(W), int(num_classes_seg)
    B = _table(kind, tab, n, fn)[-1] if kind.sources else n
    if png_out is None:
        png_out = torch.empty((B, H, W), dtype=torch.int64, device=label_u8.device)
    if onehot is None:
        onehot = torch.empty((B, H, W, ns + 1), dtype=torch.float32, device=label_u8.device)
    _tensors(fn, ((label_u8, (n, ihm, iwm), torch.uint8), (png_out, (B, H, W), torch.int64),
                  (onehot, (B, H, W, ns + 1), torch.float32), (flag, (1,), torch.int32)))
    _check(getattr(_lib, f"vrnet_{fn}_u8")(ptr(label_u8), *_table(kind, tab, n, fn), ihm, iwm, H, W, ns, ptr(png_out), ptr(onehot), ptr(flag), stream()), fn)
    return png_out, onehot


def _box_targets(kind, boxes, counts, tab, capacity, H, W, targets, counts_out, flag):
    fn = kind.name.format("box_targets")
    if boxes is None or boxes.dim() != 3:
        raise RuntimeError(f"{fn}: expected boxes ({kind.n}, max_gt, 5)")
    n, max_gt = boxes.shape[:2]
    B = _table(kind, tab, n, fn)[-1] if kind.sources else n
    if targets is None:
        targets = torch.empty((B, max_gt, 5), dtype=torch.float32, device=boxes.device)
    if counts_out is None:
        counts_out = torch.empty(B, dtype=torch.int32, device=boxes.device)
    _tensors(fn, ((boxes, (n, max_gt, 5), torch.int32), (counts, (n,), torch.int32), (targets, (B, max_gt, 5), torch.float32),
                  (counts_out, (B,), torch.int32), (flag, (1,), torch.int32)))
    _check(getattr(_lib, f"vrnet_{fn}_f32")(ptr(boxes), ptr(counts), *_table(kind, tab, n, fn), max_gt, int(capacity[0]), int(capacity[1]), int(H), int(W),
                                            ptr(targets), ptr(counts_out), ptr(flag), stream()), fn)
    return targets, counts_out


def _frames(kind, img_u8, tab, H, W, max_taps, canvas, images, flag, ws):
    fn = kind.name.format("frames")
    if img_u8 is None or img_u8.dim() != 4:
        raise RuntimeError(f"{fn}: expected frames ({kind.n}, ihm, iwm, 3)")
    n, ihm, iwm = img_u8.shape[:3]
    H, W = int(H), int(W)
    B = _table(kind, tab, n, fn)[-1] if kind.sources else n
    _tensors(fn, ((img_u8, (n, ihm, iwm, 3), torch.uint8), (canvas, (B, H, W, 3), torch.uint8), (images, (B, 3, H, W), torch.float32),
                  (flag, (1,), torch.int32)))
    need = getattr(_lib, kind.workspace)(B, ihm, iwm, H, W, int(max_taps))
    if ws is None:
        ws = _ws.get(need, img_u8.device)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise RuntimeError(f"{fn}: the workspace must be a contiguous uint8 tensor, got {ws.dtype}")
    _check(getattr(_lib, f"vrnet_{fn}_u8")(ptr(img_u8), *_table(kind, tab, n, fn), ihm, iwm, H, W, int(max_taps), ptr(canvas), ptr(images), ptr(flag),
                                           ptr(ws), ws.numel(), stream()), fn)


def _radar(kind, radar, tab, capacity, out, flag):
    fn = kind.name.format("radar")
    if radar is None or radar.dim() != 4 or radar.shape[1] != 4:
        raise RuntimeError(f"{fn}: expected radar maps ({kind.n}, 4, H, W)")
    n, _, H, W = radar.shape
    B = _table(kind, tab, n, fn)[-1] if kind.sources else n
    if out is None:
        out = torch.empty((B, 4, H, W), dtype=torch.float32, device=radar.device)
    _tensors(fn, ((radar, (n, 4, H, W), torch.float32), (out, (B, 4, H, W), torch.float32), (flag, (1,), torch.int32)))
    _check(getattr(_lib, f"vrnet_{fn}_f32")(ptr(radar), *_table(kind, tab, n, fn), int(capacity[0]), int(capacity[1]), H, W, ptr(out), ptr(flag), stream()), fn)
    return out


def seg_targets_ragged(label_u8, geom, H, W, num_classes_seg, png_out=None, onehot=None, flag=None):
    """Raw label maps of their own sizes -> the segmentation targets of the letterboxed batch (vrnet_seg_targets_ragged_u8):
    label_u8 (B,ihm,iwm) padded slots, geom the (B, GEOM_BYTES) table -> png_out (B,H,W) int64 (Pillow's NEAREST pick in the
    window, 0 outside, labels >= ns clamped to ns) and onehot (B,H,W,ns+1) f32, as `batch_formats` writes them; flag (1)
    int32 or None.  Returns (png_out, onehot)."""
    return _seg_targets(_GEOM, label_u8, geom, H, W, num_classes_seg, png_out, onehot, flag)


def box_targets_ragged(boxes, counts, geom, capacity, H, W, targets=None, counts_out=None, flag=None):
    """Boxes in pixels of the original images -> the packed targets of the letterboxed batch (vrnet_box_targets_ragged_f32):
    boxes (B,max_gt,5) int32 rows x1, y1, x2, y2, cls with counts (B) int32, geom the (B, GEOM_BYTES) table, capacity =
    (ihm, iwm) -> targets (B,max_gt,5) f32 rows [cx, cy, w, h, cls] and counts_out (B) int32, what `data.adjust_boxes` and
    `data.boxes_xyxy_to_cxcywh` give per image, kept rows in input order, the rows behind them 0.  flag (1) int32 or None:
    receives FLAG_BOX_COUNT for a count outside [0, max_gt] (clamped).  Returns (targets, counts_out)."""
    return _box_targets(_GEOM, boxes, counts, geom, capacity, H, W, targets, counts_out, flag)


def heatmap_ragged_workspace_bytes(B, H, W):
    return _lib.vrnet_heatmap_ragged_workspace(B, H, W)


# ---- training augmentation (include/vrnet_hip.h "training augmentation"): per-image records from a device table ----------
def augment_frames(img_u8, aug, H, W, max_taps, canvas=None, images=None, flag=None, ws=None):
    """Raw frames of their own sizes -> the augmented canvas (vrnet_augment_frames_u8): img_u8 (B,ihm,iwm,3) padded slots, aug
    the (B, AUG_BYTES) table -> canvas (B,H,W,3) uint8 and / or images (B,3,H,W) f32, what `data.augment_sample` and
    `device_batch` give per image; max_taps: the tap capacity of a table entry; flag (1) int32 or None; ws:
    letterbox_ragged_workspace_bytes(B, ihm, iwm, H, W, max_taps) bytes."""
    _frames(_AUG, img_u8, aug, H, W, max_taps, canvas, images, flag, ws)


def augment_seg_targets(label_u8, aug, H, W, num_classes_seg, png_out=None, onehot=None, flag=None):
    """`seg_targets_ragged` under the augmentation records (vrnet_augment_seg_targets_u8): label_u8 (B,ihm,iwm) padded slots
    -> png_out (B,H,W) int64 and onehot (B,H,W,ns+1) f32 of the augmented label canvas.  Returns (png_out, onehot)."""
    return _seg_targets(_AUG, label_u8, aug, H, W, num_classes_seg, png_out, onehot, flag)


def augment_box_targets(boxes, counts, aug, capacity, H, W, targets=None, counts_out=None, flag=None):
    """`box_targets_ragged` under the augmentation records (vrnet_augment_box_targets_f32): what `data.augment_boxes` and
    `data.boxes_xyxy_to_cxcywh` give per image.  Returns (targets, counts_out)."""
    return _box_targets(_AUG, boxes, counts, aug, capacity, H, W, targets, counts_out, flag)


def augment_radar(radar, aug, capacity, out=None, flag=None):
    """The radar maps under the augmentation records (vrnet_augment_radar_f32): radar (B,4,H,W) f32, aligned with the
    letterbox window of its frame -> out (B,4,H,W) f32, the integer gather of `data.augment_radar`; out is not radar;
    capacity = (ihm, iwm) of the frames' slots, by which the records are judged."""
    return _radar(_AUG, radar, aug, capacity, out, flag)


# ---- the blur and the rotation behind the augmentation (include/vrnet_hip.h "the blur and the rotation") ------------------------
def augment_post_frames(canvas_u8, aug, post, capacity, max_angle, images=None, canvas_out=None, flag=None):
    """The blur, the rotation and the colour stage behind `augment_frames` (vrnet_augment_post_frames_u8, one launch): canvas_u8
    (B,H,W,3), what `augment_frames` wrote with the colour stage of every record off; aug the (B, AUG_BYTES) table (its color
    and tables are applied here); post the (B, AUG_POST_BYTES) table (`data.aug_post_bytes`); capacity = (ihm, iwm) of the
    frames' slots, by which the aug records are judged; max_angle: the capacity of the rotation -> images (B,3,H,W) f32 and /
    or canvas_out (B,H,W,3) uint8, not canvas_u8: what `data.augment_sample(..., post=...)` and `device_batch` give per image."""
    fn = "augment_post_frames"
    if canvas_u8 is None or canvas_u8.dim() != 4:
        raise RuntimeError(f"{fn}: expected canvases (B, H, W, 3)")
    B, H, W = canvas_u8.shape[:3]
    _tensors(fn, ((canvas_u8, (B, H, W, 3), torch.uint8), (canvas_out, (B, H, W, 3), torch.uint8), (images, (B, 3, H, W), torch.float32),
                  (flag, (1,), torch.int32)))
    _check(_lib.vrnet_augment_post_frames_u8(ptr(canvas_u8), _table(_AUG, aug, B, fn)[0], _table(_AUG_POST, post, B, fn)[0], B,
                                             int(capacity[0]), int(capacity[1]), H, W, int(max_angle), ptr(canvas_out), ptr(images),
                                             ptr(flag), stream()), fn)


def augment_post_seg_targets(png, post, num_classes_seg, max_angle, png_out=None, onehot=None, flag=None):
    """The label canvas under the rotation (vrnet_augment_post_seg_targets_i64): png (B,H,W) int64, what `augment_seg_targets`
    wrote -> png_out (B,H,W) int64, not png, and onehot (B,H,W,ns+1) f32: `data.rotate_nearest` with fill 0.  Returns
    (png_out, onehot)."""
    fn = "augment_post_seg_targets"
    if png is None or png.dim() != 3:
        raise RuntimeError(f"{fn}: expected label canvases (B, H, W)")
    B, H, W = png.shape
    ns = int(num_classes_seg)
    if png_out is None:
        png_out = torch.empty_like(png)
    if onehot is None:
        onehot = torch.empty((B, H, W, ns + 1), dtype=torch.float32, device=png.device)
    _tensors(fn, ((png, (B, H, W), torch.int64), (png_out, (B, H, W), torch.int64), (onehot, (B, H, W, ns + 1), torch.float32),
                  (flag, (1,), torch.int32)))
    _check(_lib.vrnet_augment_post_seg_targets_i64(ptr(png), _table(_AUG_POST, post, B, fn)[0], B, H, W, ns, int(max_angle), ptr(png_out),
                                                   ptr(onehot), ptr(flag), stream()), fn)
    return png_out, onehot


def augment_post_box_targets(boxes, counts, aug, post, capacity, H, W, max_angle, targets=None, counts_out=None, flag=None):
    """`augment_box_targets` with the rotation of the post records between the flip and the clip
    (vrnet_augment_post_box_targets_f32): what `data.augment_boxes(..., post=...)` and `data.boxes_xyxy_to_cxcywh` give per image.
    Returns (targets, counts_out)."""
    fn = "augment_post_box_targets"
    if boxes is None or boxes.dim() != 3:
        raise RuntimeError(f"{fn}: expected boxes (B, max_gt, 5)")
    B, max_gt = boxes.shape[:2]
    if targets is None:
        targets = torch.empty((B, max_gt, 5), dtype=torch.float32, device=boxes.device)
    if counts_out is None:
        counts_out = torch.empty(B, dtype=torch.int32, device=boxes.device)
    _tensors(fn, ((boxes, (B, max_gt, 5), torch.int32), (counts, (B,), torch.int32), (targets, (B, max_gt, 5), torch.float32),
                  (counts_out, (B,), torch.int32), (flag, (1,), torch.int32)))
    _check(_lib.vrnet_augment_post_box_targets_f32(ptr(boxes), ptr(counts), _table(_AUG, aug, B, fn)[0], _table(_AUG_POST, post, B, fn)[0],
                                                   B, max_gt, int(capacity[0]), int(capacity[1]), int(H), int(W), int(max_angle),
                                                   ptr(targets), ptr(counts_out), ptr(flag), stream()), fn)
    return targets, counts_out


def augment_post_radar(radar, post, max_angle, out=None, flag=None):
    """A finished radar input under the rotation (vrnet_augment_post_radar_f32): radar (B,4,H,W) f32, what `augment_radar` or
    `radar_map` wrote -> out (B,4,H,W) f32, not radar: `data.rotate_nearest` per channel with fill 0.0."""
    fn = "augment_post_radar"
    if radar is None or radar.dim() != 4 or radar.shape[1] != 4:
        raise RuntimeError(f"{fn}: expected radar maps (B, 4, H, W)")
    B, _, H, W = radar.shape
    if out is None:
        out = torch.empty_like(radar)
    _tensors(fn, ((radar, (B, 4, H, W), torch.float32), (out, (B, 4, H, W), torch.float32), (flag, (1,), torch.int32)))
    _check(_lib.vrnet_augment_post_radar_f32(ptr(radar), _table(_AUG_POST, post, B, fn)[0], B, H, W, int(max_angle), ptr(out), ptr(flag),
                                             stream()), fn)
    return out


# ---- Mosaic (include/vrnet_hip.h "Mosaic on the device"): one record per OUTPUT image, S source slots --------------------------
def mosaic_workspace_bytes(B, ihm, iwm, H, W, max_taps):
    return _lib.vrnet_mosaic_workspace_bytes(B, ihm, iwm, H, W, max_taps)


def mosaic_frames(img_u8, mosaic, H, W, max_taps, canvas=None, images=None, flag=None, ws=None):
    """S raw source frames -> B Mosaic canvases (vrnet_mosaic_frames_u8): img_u8 (S,ihm,iwm,3) padded slots, mosaic the
    (B, MOSAIC_BYTES) table -> canvas (B,H,W,3) uint8 and / or images (B,3,H,W) f32, what `data.mosaic_sample` and
    `device_batch` give per output image; max_taps: the tap capacity of a table entry; flag (1) int32 or None; ws:
    mosaic_workspace_bytes(B, ihm, iwm, H, W, max_taps) bytes.  No host validation: `data.check_mosaic_table` is the
    caller's."""
    _frames(_MOSAIC, img_u8, mosaic, H, W, max_taps, canvas, images, flag, ws)


def mosaic_seg_targets(label_u8, mosaic, H, W, num_classes_seg, png_out=None, onehot=None, flag=None):
    """`augment_seg_targets` under Mosaic records (vrnet_mosaic_seg_targets_u8): label_u8 (S,ihm,iwm) padded slots -> png_out
    (B,H,W) int64 and onehot (B,H,W,ns+1) f32 of the Mosaic label canvas.  Returns (png_out, onehot)."""
    return _seg_targets(_MOSAIC, label_u8, mosaic, H, W, num_classes_seg, png_out, onehot, flag)


def mosaic_box_targets(boxes, counts, mosaic, capacity, H, W, targets=None, counts_out=None, flag=None):
    """The boxes of S sources -> the packed targets of B Mosaic images (vrnet_mosaic_box_targets_f32): what
    `data.mosaic_boxes` and `data.boxes_xyxy_to_cxcywh` give per output image, in tile-then-row order; of more than max_gt
    kept rows the first max_gt stay and flag receives FLAG_BOX_COUNT.  Returns (targets, counts_out)."""
    return _box_targets(_MOSAIC, boxes, counts, mosaic, capacity, H, W, targets, counts_out, flag)


def mosaic_radar(radar, mosaic, capacity, out=None, flag=None):
    """The radar maps of S sources under Mosaic records (vrnet_mosaic_radar_f32): radar (S,4,H,W) f32, each aligned with the
    letterbox window of its source -> out (B,4,H,W) f32, the integer gather of `data.mosaic_sample`; out is not radar;
    capacity = (ihm, iwm) of the frames' slots, by which the records are judged."""
    return _radar(_MOSAIC, radar, mosaic, capacity, out, flag)


# ---- the radar map from 4D radar points (include/vrnet_hip.h "the radar map from 4D radar points") -------------------------
RADAR_VIEW_BYTES = 80    # sizeof(vrnet_radar_view)
FLAG_POINT_COUNT = 1024  # VR_FLAG_POINT_COUNT of csrc/common.h: radar_map clamped a count outside [0, max_points]
RADAR_MAX_RADIUS = 8


def _views(views, B, fn):
    """The table: a contiguous uint8 GPU tensor (B, RADAR_VIEW_BYTES), 8-byte aligned (`data.radar_views` packs it)."""
    if views is None or views.dtype != torch.uint8 or tuple(views.shape) != (B, RADAR_VIEW_BYTES) or not views.is_contiguous() or \
            not views.is_cuda or views.data_ptr() % 8:
        raise RuntimeError(f"{fn}: the view table must be a contiguous, 8-byte aligned uint8 GPU tensor of shape ({B}, {RADAR_VIEW_BYTES})")
    return ptr(views)


def radar_map_workspace_bytes(B, H, W):
    return _lib.vrnet_radar_map_workspace(B, H, W)


def _radar_map(fn, points, views, H, W, radius, min_depth, out, flag, ws, post=None, max_angle=0):
    """`radar_map` and `radar_map_post`: one body, the post table optional."""
    if points is None or points.dim() != 3 or points.shape[2] != 7 or points.shape[1] < 1:
        raise RuntimeError(f"{fn}: expected points (B, max_points, 7)")
    B, max_points = points.shape[:2]
    H, W = int(H), int(W)
    _tensors(fn, ((points, (B, max_points, 7), torch.float32), (out, (B, 4, H, W), torch.float32), (flag, (1,), torch.int32)))
    if out is None:
        raise RuntimeError(f"{fn}: out is required")
    need = _lib.vrnet_radar_map_workspace(B, H, W)
    if ws is None:
        ws = _ws.get(need, points.device)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise RuntimeError(f"{fn}: the workspace must be a contiguous uint8 tensor, got {ws.dtype}")
    head = (ptr(points), max_points, _views(views, B, fn), B, H, W, int(radius), float(min_depth))
    tail = (ptr(out), ptr(flag), ptr(ws), ws.numel(), stream())
    if post is None:
        _check(_lib.vrnet_radar_map_f32(*head, *tail), fn)
    else:
        _check(_lib.vrnet_radar_map_post_f32(*head, _table(_AUG_POST, post, B, fn)[0], int(max_angle), *tail), fn)
    return out


def radar_map(points, views, H, W, radius, min_depth, out, flag=None, ws=None):
    """Radar points -> the network's radar input (vrnet_radar_map_f32): points (B, max_points, 7) f32 rows x, y, z, f0..f3,
    views the (B, RADAR_VIEW_BYTES) table -> out (B, 4, H, W) f32, what `data.radar_map` gives per image, bit for bit; radius
    0..8, min_depth > 0; flag (1) int32 or None: FLAG_GEOMETRY for a record without pixels, FLAG_POINT_COUNT for a clamped
    count; ws: radar_map_workspace_bytes(B, H, W) bytes.  Three launches.  Returns out."""
    return _radar_map("radar_map", points, views, H, W, radius, min_depth, out, flag, ws)


def radar_map_post(points, views, post, H, W, radius, min_depth, max_angle, out, flag=None, ws=None):
    """`radar_map` under the rotation of the post stage (vrnet_radar_map_post_f32): post the (B, AUG_POST_BYTES) table
    (`data.aug_post_bytes`), max_angle the capacity its records are judged by -> out (B, 4, H, W) f32, what
    `data.radar_map(..., post=)` gives per image, bit for bit: the centre of every kept point goes through the record's
    forward matrix once, its cut footprint follows it.  flag receives FLAG_GEOMETRY also for a post record that is not finite
    or above max_angle (that image is then not rotated).  The same three launches and workspace.  Returns out."""
    if post is None:
        raise RuntimeError("radar_map_post: the post table is required (radar_map is the call without one)")
    return _radar_map("radar_map_post", points, views, H, W, radius, min_depth, out, flag, ws, post, max_angle)


# ---- the radar readout of the detections (include/vrnet_hip.h "the radar readout of the detections") -------------------------
def box_radar_workspace_bytes(B, max_points):
    return _lib.vrnet_box_radar_workspace(B, max_points)


def box_radar(points, views, rows, kept, min_depth, shrink, counts, readout, flag=None, ws=None):
    """Radar points and kept detections -> the readout of every box (vrnet_box_radar_f32): points (B, max_points, 7) f32 and
    views (B, RADAR_VIEW_BYTES) as `radar_map` takes them (ih, iw, count and P are read), rows (B, cap, 7) f32 with top, left,
    bottom, right in pixels of the original frame in front, kept (B) int32 -> counts (B, cap) int32 and readout (B, cap, 2, 5)
    f32, what `data.box_radar` gives per image on rows[:kept], bit for bit, and zeros from row kept[b] on: every element is
    written.  min_depth > 0, 0 < shrink <= 1; flag (1) int32 or None: FLAG_GEOMETRY for ih or iw <= 0 (zeros for that image),
    FLAG_POINT_COUNT / FLAG_BOX_COUNT for a clamped count / kept; ws: box_radar_workspace_bytes(B, max_points) bytes.  Two
    launches.  Returns (counts, readout)."""
    fn = "box_radar"
    if points is None or points.dim() != 3 or points.shape[2] != 7 or points.shape[1] < 1:
        raise RuntimeError(f"{fn}: expected points (B, max_points, 7)")
    B, max_points = points.shape[:2]
    if rows is None or rows.dim() != 3 or rows.shape[0] != B or rows.shape[1] < 1 or rows.shape[2] != 7:
        raise RuntimeError(f"{fn}: expected rows ({B}, cap, 7)")
    cap = rows.shape[1]
    if counts is None or readout is None:
        raise RuntimeError(f"{fn}: counts and readout are required")
    _tensors(fn, ((points, (B, max_points, 7), torch.float32), (rows, (B, cap, 7), torch.float32), (kept, (B,), torch.int32),
                  (counts, (B, cap), torch.int32), (readout, (B, cap, 2, 5), torch.float32), (flag, (1,), torch.int32)))
    if kept is None:
        raise RuntimeError(f"{fn}: kept is required")
    need = _lib.vrnet_box_radar_workspace(B, max_points)
    if ws is None:
        ws = _ws.get(need, points.device)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise RuntimeError(f"{fn}: the workspace must be a contiguous uint8 tensor, got {ws.dtype}")
    _check(_lib.vrnet_box_radar_f32(ptr(points), max_points, _views(views, B, fn), B, ptr(rows), ptr(kept), cap, float(min_depth),
                                    float(shrink), ptr(counts), ptr(readout), ptr(flag), ptr(ws), ws.numel(), stream()), fn)
    return counts, readout


# ---- multi-object tracking of the detections (include/vrnet_hip.h "multi-object tracking of the detections") -----------------
TRACK_WORDS, TRACK_HEAD = 16, 4  # sizeof(vrnet_track) / 4; the int32 words of a stream's header


def track_update(rows, kept, table, head, ids, params, box_points=None, box_radar=None, flag=None):
    """One call of the tracker on every stream (vrnet_track_update_f32, one launch): rows (B, cap, 7) f32 and kept (B) int32 as
    `detect_finish` writes them, cap <= 1024; table (B, T, 16) int32, the (B, T) vrnet_track records of `data.TRACK_DTYPE` as
    words, T in [1, 256], and head (B, 4) int32: the state, updated in place (zeros: the reset state); ids (B, cap) int32, the
    track id of every row, every element written; params: the dict of `data.check_track_params` (iou, max_age, gain,
    range_gain; max_tracks is the table's T).  box_points (B, cap) int32 and box_radar (B, cap, 2, 5) f32: the outputs of
    `box_radar` for these rows, both or neither.  flag (1) int32 or None: FLAG_BOX_COUNT for a clamped kept, 32768
    (data.FLAG_TRACK_FULL) for a valid row that found no free slot.  What `data.track_update` gives, bit for bit.  Returns
    (table, head, ids)."""
    fn = "track_update"
    if rows is None or rows.dim() != 3 or rows.shape[1] < 1 or rows.shape[2] != 7:
        raise RuntimeError(f"{fn}: expected rows (B, cap, 7)")
    B, cap = rows.shape[:2]
    if table is None or table.dim() != 3 or table.shape[0] != B or table.shape[1] < 1 or table.shape[2] != TRACK_WORDS:
        raise RuntimeError(f"{fn}: expected table ({B}, max_tracks, {TRACK_WORDS}) int32, the records as words")
    T = table.shape[1]
    if kept is None or head is None or ids is None:
        raise RuntimeError(f"{fn}: kept, head and ids are required")
    if (box_points is None) != (box_radar is None):
        raise RuntimeError(f"{fn}: box_points and box_radar come together or not at all")
    _tensors(fn, ((rows, (B, cap, 7), torch.float32), (kept, (B,), torch.int32), (table, (B, T, TRACK_WORDS), torch.int32),
                  (head, (B, TRACK_HEAD), torch.int32), (ids, (B, cap), torch.int32), (box_points, (B, cap), torch.int32),
                  (box_radar, (B, cap, 2, 5), torch.float32), (flag, (1,), torch.int32)))
    try:
        iou, max_age, (gp, gv), (rp, rv) = params["iou"], params["max_age"], params["gain"], params["range_gain"]
    except (TypeError, KeyError, ValueError):
        raise RuntimeError(f"{fn}: params is the dict of data.check_track_params") from None
    _check(_lib.vrnet_track_update_f32(ptr(rows), ptr(kept), B, cap, ptr(table), T, ptr(head), ptr(ids), ptr(box_points),
                                       ptr(box_radar), float(iou), int(max_age), float(gp), float(gv), float(rp), float(rv),
                                       ptr(flag), stream()), fn)
    return table, head, ids


# ---- radar points under Mosaic (include/vrnet_hip.h "radar points under Mosaic") ----------------------------------------------
RADAR_SOURCE_BYTES = 56  # sizeof(vrnet_radar_source)


def mosaic_radar_points_workspace_bytes(B, H, W):
    return _lib.vrnet_mosaic_radar_points_workspace(B, H, W)


def mosaic_radar_points(points, sources, table, capacity, H, W, radius, min_depth, out, flag=None, ws=None):
    """The radar points of S sources -> the radar input of B Mosaic images (vrnet_mosaic_radar_points_f32): points
    (S, max_points, 7) f32 rows x, y, z, f0..f3, sources the (S, RADAR_SOURCE_BYTES) table of counts and projections
    (`data.radar_sources` packs it), table the (B, MOSAIC_BYTES) Mosaic table the other Mosaic calls take, capacity = (ihm, iwm)
    of the frames' slots, by which the records are judged -> out (B, 4, H, W) f32, what `data.mosaic_radar_map` gives per output
    image, bit for bit; radius 0..8, min_depth > 0; flag (1) int32 or None: FLAG_GEOMETRY for a record that had to be clamped
    (its whole image is 0), FLAG_POINT_COUNT for a clamped count; ws: mosaic_radar_points_workspace_bytes(B, H, W) bytes.
    Three launches.  Returns out."""
    fn = "mosaic_radar_points"
    if points is None or points.dim() != 3 or points.shape[2] != 7 or points.shape[1] < 1:
        raise RuntimeError(f"{fn}: expected points (S, max_points, 7)")
    S, max_points = points.shape[:2]
    H, W = int(H), int(W)
    if sources is None or sources.dtype != torch.uint8 or tuple(sources.shape) != (S, RADAR_SOURCE_BYTES) or \
            not sources.is_contiguous() or not sources.is_cuda or sources.data_ptr() % 8:
        raise RuntimeError(f"{fn}: the source table must be a contiguous, 8-byte aligned uint8 GPU tensor of shape ({S}, {RADAR_SOURCE_BYTES})")
    _, tab, B = _table(_MOSAIC, table, S, fn)
    if out is None:
        raise RuntimeError(f"{fn}: out is required")
    _tensors(fn, ((points, (S, max_points, 7), torch.float32), (out, (B, 4, H, W), torch.float32), (flag, (1,), torch.int32)))
    need = _lib.vrnet_mosaic_radar_points_workspace(B, H, W)
    if ws is None:
        ws = _ws.get(need, points.device)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise RuntimeError(f"{fn}: the workspace must be a contiguous uint8 tensor, got {ws.dtype}")
    _check(_lib.vrnet_mosaic_radar_points_f32(ptr(points), max_points, S, ptr(sources), tab, B, int(capacity[0]), int(capacity[1]), H, W,
                                              int(radius), float(min_depth), ptr(out), ptr(flag), ptr(ws), ws.numel(), stream()), fn)
    return out


# ---- class names and scores on the rendered detections (csrc/labels.hip) ---------------------------------------------------
FLAG_LABEL_SCORE = 2048  # LB_FLAG_SCORE of csrc/labels.hip: a score that is NaN or outside [0, 1], clamped
LABEL_SCORES = 101       # the strings 0.00 .. 1.00
LABEL_RECORD = 8         # int32 per atlas record


def label_index(rows, kept, offsets, num_classes, label_idx, flag=None):
    """The kept rows (B, cap, 7) `detect_finish[_ragged]` wrote, with kept (B) and offsets (B + 1) -> label_idx (N) int32,
    class * 101 + k at offsets[b] + r for every kept row (vrnet_label_index_f32); flag (1) int32 or None."""
    if rows is None or rows.dim() != 3:
        raise RuntimeError("label_index: expected rows of shape (B, cap, 7)")
    B, cap = rows.shape[:2]
    if label_idx is None or label_idx.dim() != 1:
        raise RuntimeError("label_index: label_idx must be a 1-D int32 tensor")
    _tensors("label_index", ((rows, (B, cap, 7), torch.float32), (kept, (B,), torch.int32), (offsets, (B + 1,), torch.int32),
                             (label_idx, (label_idx.shape[0],), torch.int32), (flag, (1,), torch.int32)))
    if kept is None or offsets is None:
        raise RuntimeError("label_index: kept and offsets are required")
    _check(_lib.vrnet_label_index_f32(ptr(rows), ptr(kept), ptr(offsets), B, cap, int(num_classes), ptr(label_idx),
                                      label_idx.shape[0], ptr(flag), stream()), "label_index")


def render_labels(picture, boxes, box_offsets, box_palette, thickness, label_idx, blob, records, size_index, flag=None, geom=None,
                  fn="render_labels"):
    """Tags and label text over the picture `render` finished, in place (vrnet_render_labels_u8): picture (B,ih,iw,3) uint8,
    boxes (N,5) / box_offsets (B+1) / box_palette (m,3) / thickness as `render` took them, label_idx (N) int32 = class * 101
    + k, blob (bytes) uint8 and records (sizes, num_classes * 101, 8) int32 of a `render.LabelAtlas`, size_index its font size.
    With geom (`_table_call`) thickness is None: ih, iw and the thickness of image b come from geom[b], and size_index is the
    (B) int32 device table of each image's font size, -1 for an image without labels (vrnet_render_labels_ragged_u8)."""
    table = _table_call(fn, geom, (("thickness", thickness, None),))
    if picture is None or picture.dim() != 4 or picture.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected a contiguous uint8 picture of shape (B, ih, iw, 3)")
    B, ih, iw = picture.shape[:3]
    if boxes is None or box_offsets is None or box_palette is None or label_idx is None or blob is None or records is None:
        raise RuntimeError(f"{fn}: boxes, box_offsets, box_palette, label_idx and the atlas blob and records are required")
    if records.dim() != 3 or records.shape[0] < 1 or records.shape[1] < LABEL_SCORES or records.shape[1] % LABEL_SCORES:
        raise RuntimeError(f"{fn}: the atlas records must have shape (sizes, num_classes * {LABEL_SCORES}, {LABEL_RECORD}), got "
                           f"{tuple(records.shape)}")
    n_rows, n_sizes = boxes.shape[0], records.shape[0]
    _tensors(fn, ((picture, (B, ih, iw, 3), torch.uint8), (boxes, (n_rows, 5), torch.int32), (box_offsets, (B + 1,), torch.int32),
                  (box_palette, (box_palette.shape[0], 3), torch.uint8), (label_idx, (n_rows,), torch.int32),
                  (blob, (blob.shape[0],), torch.uint8), (records, (n_sizes, records.shape[1], LABEL_RECORD), torch.int32),
                  (flag, (1,), torch.int32), (size_index if table else None, (B,), torch.int32)))
    if table and size_index is None:
        raise RuntimeError(f"{fn}: the per-image size-index table is required")
    if n_rows == 0:                           # nothing to draw (and an empty tensor has no address to pass)
        return
    rows = (ptr(boxes), ptr(box_offsets), n_rows, ptr(box_palette), box_palette.shape[0])
    atlas = (ptr(label_idx), ptr(blob), blob.shape[0], ptr(records), records.shape[1] // LABEL_SCORES, n_sizes)
    if table:
        _check(_lib.vrnet_render_labels_ragged_u8(ptr(picture), _geom(geom, B, fn), ptr(size_index), B, ih, iw, *rows, *atlas, ptr(flag),
                                                  stream()), fn)
    else:
        _check(_lib.vrnet_render_labels_u8(ptr(picture), B, ih, iw, *rows, int(thickness), *atlas, int(size_index), ptr(flag),
                                           stream()), fn)


def render_labels_ragged(picture, geom, size_index, boxes, box_offsets, box_palette, label_idx, blob, records, flag=None):
    render_labels(picture, boxes, box_offsets, box_palette, None, label_idx, blob, records, size_index, flag, geom, "render_labels_ragged")


# ---- track ids, radar range and closing speed under the rendered detections (csrc/captions.hip) ------------------------------
FLAG_CAPTION = 65536     # VR_FLAG_CAPTION of csrc/common.h: a range or a speed that cannot be drawn, left out of its caption
CAPTION_WORDS = 12       # int32 per caption record: 32 codes as bytes, their count, three zeros
CAPTION_GLYPHS = 18      # "0123456789.-+#m/s "
GLYPH_RECORD = 4         # int32 per glyph record: blob offset, cell width, cell height, 0


def caption_text(kept, offsets, captions, ids=None, table=None, box_points=None, box_radar=None, rate_scale=0.0, flag=None):
    """The caption of every kept row, composed on the device (vrnet_caption_text_f32, one launch): kept (B) and offsets (B + 1)
    int32 as `detect_finish` writes them -> captions (N, 12) int32 records at offsets[b] + r, nothing else written.  ids (B, cap)
    int32 and table (B, T, 16) int32 of `track_update`, box_points (B, cap) int32 and box_radar (B, cap, 2, 5) f32 of
    `box_radar`: each optional, table needs ids, at least one of ids and the readout.  rate_scale: the frame rate that turns the
    tracker's per-call range rate into the closing speed, 0 for no speed field.  flag (1) int32 or None: FLAG_CAPTION for a
    field left out, FLAG_BOX_COUNT for a clamped kept.  What `render.caption_strings` gives, code for code.  Returns captions."""
    fn = "caption_text"
    if kept is None or offsets is None or captions is None:
        raise RuntimeError(f"{fn}: kept, offsets and captions are required")
    if (box_points is None) != (box_radar is None):
        raise RuntimeError(f"{fn}: box_points and box_radar come together or not at all")
    shaped = ids if ids is not None else box_points
    if shaped is None or shaped.dim() != 2:
        raise RuntimeError(f"{fn}: needs track ids (B, cap) or the radar readout")
    if table is not None and (ids is None or table.dim() != 3 or table.shape[2] != TRACK_WORDS):
        raise RuntimeError(f"{fn}: a track table (B, max_tracks, {TRACK_WORDS}) int32 needs the track ids")
    if captions.dim() != 2:
        raise RuntimeError(f"{fn}: captions must have shape (N, {CAPTION_WORDS})")
    B, cap = shaped.shape
    T = table.shape[1] if table is not None else 0
    _tensors(fn, ((ids, (B, cap), torch.int32), (kept, (B,), torch.int32), (offsets, (B + 1,), torch.int32),
                  (table, (B, T, TRACK_WORDS), torch.int32), (box_points, (B, cap), torch.int32),
                  (box_radar, (B, cap, 2, 5), torch.float32), (captions, (captions.shape[0], CAPTION_WORDS), torch.int32),
                  (flag, (1,), torch.int32)))
    if captions.shape[0] == 0:                # nothing to write (and an empty tensor has no address to pass)
        return captions
    _check(_lib.vrnet_caption_text_f32(ptr(ids), ptr(kept), ptr(offsets), B, cap, ptr(table), T, ptr(box_points), ptr(box_radar),
                                       float(rate_scale), ptr(captions), captions.shape[0], ptr(flag), stream()), fn)
    return captions


def render_captions(picture, boxes, box_offsets, box_palette, captions, blob, records, size_index, flag=None, geom=None,
                    fn="render_captions"):
    """Caption tags and text over the finished picture, in place (vrnet_render_captions_u8): picture (B,ih,iw,3) uint8, boxes
    (N,5) / box_offsets (B+1) / box_palette (m,3) as `render` took them, captions (N, 12) int32 as `caption_text` writes them,
    blob (bytes) uint8 and records (sizes, 18, 4) int32 of a `render.GlyphAtlas`, size_index its font size.  With geom
    (`_table_call`) ih and iw of image b come from geom[b], and size_index is the (B) int32 device table of each image's font
    size, -1 for an image without captions (vrnet_render_captions_ragged_u8)."""
    table = _table_call(fn, geom)
    if picture is None or picture.dim() != 4 or picture.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected a contiguous uint8 picture of shape (B, ih, iw, 3)")
    B, ih, iw = picture.shape[:3]
    if boxes is None or box_offsets is None or box_palette is None or captions is None or blob is None or records is None:
        raise RuntimeError(f"{fn}: boxes, box_offsets, box_palette, captions and the atlas blob and records are required")
    if records.dim() != 3 or records.shape[0] < 1:
        raise RuntimeError(f"{fn}: the atlas records must have shape (sizes, {CAPTION_GLYPHS}, {GLYPH_RECORD}), got {tuple(records.shape)}")
    if torch.is_tensor(size_index) != table:
        raise RuntimeError(f"{fn}: size_index is one font size of the atlas, or beside a geometry table the (B) int32 table of them")
    n_rows, n_sizes = boxes.shape[0], records.shape[0]
    _tensors(fn, ((picture, (B, ih, iw, 3), torch.uint8), (boxes, (n_rows, 5), torch.int32), (box_offsets, (B + 1,), torch.int32),
                  (box_palette, (box_palette.shape[0], 3), torch.uint8), (captions, (n_rows, CAPTION_WORDS), torch.int32),
                  (blob, (blob.shape[0],), torch.uint8), (records, (n_sizes, CAPTION_GLYPHS, GLYPH_RECORD), torch.int32),
                  (flag, (1,), torch.int32), (size_index if table else None, (B,), torch.int32)))
    if n_rows == 0:                           # nothing to draw (and an empty tensor has no address to pass)
        return
    rows = (ptr(boxes), ptr(box_offsets), n_rows, ptr(box_palette), box_palette.shape[0])
    atlas = (ptr(captions), ptr(blob), blob.shape[0], ptr(records), n_sizes)
    if table:
        _check(_lib.vrnet_render_captions_ragged_u8(ptr(picture), _geom(geom, B, fn), ptr(size_index), B, ih, iw, *rows, *atlas,
                                                    ptr(flag), stream()), fn)
    else:
        _check(_lib.vrnet_render_captions_u8(ptr(picture), B, ih, iw, *rows, *atlas, int(size_index), ptr(flag), stream()), fn)


# ---- detection crops (csrc/crops.hip) ----------------------------------------------------------------------------------------
FLAG_CROP_ARENA = 4096   # VR_FLAG_CROP_ARENA of csrc/common.h: a crop that did not fit into the arena, dropped
CROP_RECORD = 4          # int32 per vrnet_crop_rec: offset, w, h, image


def crop_boxes(frames, rows, offsets, arena, table, summary, geom=None, flag=None):
    """The crops of yolo.py:180-193 into one packed arena (vrnet_crop_boxes_u8): frames (B, ihm, iwm, 3) uint8, rows (n_cap, 5)
    / offsets (B + 1) int32 as `detect_finish[_ragged]` leave them -> arena (3 * capacity) uint8, table (n_cap, 4) int32 records
    offset, w, h, image and summary (2) int32 = (rows, pixels in use), by the rule of `render.crop_layout`; geom: the
    (B, GEOM_BYTES) table of a ragged batch, None: every image fills its slot; flag (1) int32 or None: FLAG_CROP_ARENA for a
    dropped crop, FLAG_GEOMETRY for a clamped record.  Two launches."""
    fn = "crop_boxes"
    if frames is None or frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected contiguous uint8 frames of shape (B, ihm, iwm, 3)")
    B, ihm, iwm = frames.shape[:3]
    if rows is None or rows.dim() != 2 or rows.shape[0] < 1 or offsets is None or arena is None or table is None or summary is None:
        raise RuntimeError(f"{fn}: rows (n_cap >= 1, 5), offsets, arena, table and summary are required")
    n_cap = rows.shape[0]
    if arena.dim() != 1 or arena.shape[0] < 3 or arena.shape[0] % 3:
        raise RuntimeError(f"{fn}: the arena must be a 1-D uint8 tensor of 3 * capacity bytes, got shape {tuple(arena.shape)}")
    _tensors(fn, ((frames, (B, ihm, iwm, 3), torch.uint8), (rows, (n_cap, 5), torch.int32), (offsets, (B + 1,), torch.int32),
                  (arena, (arena.shape[0],), torch.uint8), (table, (n_cap, CROP_RECORD), torch.int32),
                  (summary, (2,), torch.int32), (flag, (1,), torch.int32)))
    _check(_lib.vrnet_crop_boxes_u8(ptr(frames), B, ihm, iwm, None if geom is None else _geom(geom, B, fn), ptr(rows), ptr(offsets),
                                    n_cap, ptr(arena), arena.shape[0] // 3, ptr(table), ptr(summary), ptr(flag), stream()), fn)


# ---- fixed-size detection chips (csrc/chips.hip) -----------------------------------------------------------------------------
CHIP_RECORD = 8          # int32 per vrnet_chip_rec: image, w, h, nw, nh, dx, dy, state
CHIP_MAX = 256           # the largest side of a chip


def chip_workspace_bytes(n_cap, sh, sw):
    n = _lib.vrnet_chip_workspace(n_cap, sh, sw)
    if n < 0:
        raise RuntimeError(f"chip_boxes: bad shape ({n_cap} rows, chips of {sh} x {sw}; 1..2^20 rows, sides in 1..{CHIP_MAX})")
    return n


def chip_boxes(frames, rows, offsets, chips, table, summary, ws, letterbox=False, chips_f32=None, geom=None, flag=None):
    """The crops of `crop_boxes` brought to one size (vrnet_chip_boxes_u8): frames (B, ihm, iwm, 3) uint8, rows (n_cap, 5) /
    offsets (B + 1) int32 as `detect_finish[_ragged]` leave them -> chips (n_cap, sh, sw, 3) uint8, chip n of row n, by the rule
    of `render.chip_boxes_host` (Pillow's BICUBIC on the crop; letterbox: resize_image's window on grey 128); chips_f32
    (n_cap, 3, sh, sw) float32 or None: the normalised form; table (n_cap, 8) int32 records image, w, h, nw, nh, dx, dy, state
    and summary (1) int32 = rows; ws: uint8, at least `chip_workspace_bytes(n_cap, sh, sw)`; geom: the (B, GEOM_BYTES) table of
    a ragged batch, None: every image fills its slot; flag (1) int32 or None: FLAG_GEOMETRY for a clamped record.  Chips behind
    the last row are not written.  Two launches."""
    fn = "chip_boxes"
    if frames is None or frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected contiguous uint8 frames of shape (B, ihm, iwm, 3)")
    B, ihm, iwm = frames.shape[:3]
    if rows is None or rows.dim() != 2 or rows.shape[0] < 1 or offsets is None or chips is None or table is None or summary is None:
        raise RuntimeError(f"{fn}: rows (n_cap >= 1, 5), offsets, chips, table and summary are required")
    n_cap = rows.shape[0]
    if chips.dim() != 4 or chips.shape[0] != n_cap or chips.shape[3] != 3 or not (1 <= chips.shape[1] <= CHIP_MAX and
                                                                                  1 <= chips.shape[2] <= CHIP_MAX):
        raise RuntimeError(f"{fn}: the chips must be a uint8 tensor ({n_cap}, sh, sw, 3) with sides in 1..{CHIP_MAX}, got shape "
                           f"{tuple(chips.shape)}")
    sh, sw = chips.shape[1:3]
    need = chip_workspace_bytes(n_cap, sh, sw)
    if ws is None or ws.dtype != torch.uint8 or ws.dim() != 1 or ws.shape[0] < need or not ws.is_contiguous():
        raise RuntimeError(f"{fn}: the workspace must be a contiguous uint8 tensor of at least {need} bytes")
    _tensors(fn, ((frames, (B, ihm, iwm, 3), torch.uint8), (rows, (n_cap, 5), torch.int32), (offsets, (B + 1,), torch.int32),
                  (chips, (n_cap, sh, sw, 3), torch.uint8), (chips_f32, (n_cap, 3, sh, sw), torch.float32),
                  (table, (n_cap, CHIP_RECORD), torch.int32), (summary, (1,), torch.int32), (flag, (1,), torch.int32)))
    _check(_lib.vrnet_chip_boxes_u8(ptr(frames), B, ihm, iwm, None if geom is None else _geom(geom, B, fn), ptr(rows), ptr(offsets),
                                    n_cap, sh, sw, int(bool(letterbox)), ptr(chips), ptr(chips_f32), ptr(table), ptr(summary),
                                    ptr(ws), ptr(flag), stream()), fn)


# ---- baseline JPEG (csrc/jpeg.hip) ---------------------------------------------------------------------------------------------
FLAG_JPEG_ARENA = 262144     # VR_FLAG_JPEG_ARENA of csrc/common.h: a file that did not fit its slot of the arena, length 0
JPEG_HEADER = 623            # bytes in front of the scan data
JPEG_MAX_BLOCKS = 1 << 20    # JP_MAX_BLOCKS of csrc/jpeg.hip: the blocks of one slot, so that bit offsets fit 32 bits


def jpeg_workspace_bytes(B, H, W, subsampling, capacity):
    n = _lib.vrnet_jpeg_workspace_bytes(B, H, W, int(subsampling), int(capacity))
    if n < 0:
        raise RuntimeError(f"jpeg_encode: bad shape (B {B}, slots of {H} x {W}, subsampling {subsampling}, capacity {capacity}; "
                           f"1..65535 images, sides up to 65535, at most {JPEG_MAX_BLOCKS} blocks an image, subsampling 0 or 2, a "
                           f"capacity from {JPEG_HEADER + 2} bytes to below 2^31)")
    return n


def jpeg_encode(images, header, arena, record, ws, subsampling=0, sizes=None, geom=None, flag=None):
    """Baseline JPEG files by the rule of `render.jpeg_encode_host` (vrnet_jpeg_encode_u8): images (B, H, W, 3) uint8 -> arena
    (B, capacity) uint8, slot b a complete file in its first record[b, 0] bytes, and record (B, 2) int32 = (length, state):
    state 1 a file, 2 it did not fit the capacity (length 0, FLAG_JPEG_ARENA), 3 an image without pixels (length 0).  Bytes of
    a slot behind its length are not defined.  header: the (623) uint8 template of `render.jpeg_header` on the device, which
    holds the quantisation tables; height and width are patched per image.  sizes: a (B, 2) int32 device table (h, w) of the
    images in the corners of their slots, or geom (`_table_call`): the (B, GEOM_BYTES) table of a ragged batch; neither: every
    image fills its slot.  ws: uint8, at least jpeg_workspace_bytes(B, H, W, subsampling, capacity) bytes; flag (1) int32 or
    None: FLAG_JPEG_ARENA, and FLAG_GEOMETRY for a size that had to be clamped.  Eight launches, no host synchronisation."""
    fn = "jpeg_encode"
    table_call = _table_call(fn, geom, (("sizes", sizes, None),))
    if images is None or images.dim() != 4 or images.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected contiguous uint8 images of shape (B, H, W, 3)")
    B, H, W = images.shape[:3]
    if arena is None or arena.dim() != 2 or header is None or record is None or ws is None:
        raise RuntimeError(f"{fn}: header, arena (B, capacity), record and the workspace are required")
    capacity = arena.shape[1]
    need = jpeg_workspace_bytes(B, H, W, subsampling, capacity)
    if ws.dtype != torch.uint8 or ws.dim() != 1 or ws.shape[0] < need or not ws.is_contiguous():
        raise RuntimeError(f"{fn}: the workspace must be a contiguous uint8 tensor of at least {need} bytes")
    _tensors(fn, ((images, (B, H, W, 3), torch.uint8), (header, (JPEG_HEADER,), torch.uint8), (arena, (B, capacity), torch.uint8),
                  (record, (B, 2), torch.int32), (sizes, (B, 2), torch.int32), (flag, (1,), torch.int32)))
    _check(_lib.vrnet_jpeg_encode_u8(ptr(images), B, H, W, _geom(geom, B, fn) if table_call else None, ptr(sizes), int(subsampling),
                                     ptr(header), ptr(arena), capacity, ptr(record), ptr(flag), ptr(ws), ws.numel(), stream()), fn)


# ---- connected regions of the class map (csrc/regions.hip) ---------------------------------------------------------------------
FLAG_REGIONS = 131072    # VR_FLAG_REGIONS of csrc/common.h: more regions than the table holds; labels and head are complete
REGION_WORDS = 12        # int32 per vrnet_region: cls, area, left, top, right, bottom, first, det, then sum_x and sum_y as int64
REGION_HEAD = 4          # int32 per image: regions, records in the table, pixels in kept regions, pixels dropped by min_area


def seg_regions_workspace_bytes(B, ihm, iwm):
    n = _lib.vrnet_seg_regions_workspace_bytes(B, ihm, iwm)
    if n < 0:
        raise RuntimeError(f"seg_regions: bad shape (B {B}, slots of {ihm} x {iwm}; 1..65535 images, sides up to 2^17, below 2^31 "
                           "pixels each)")
    return n


def seg_regions(class_map, rows, offsets, labels, table, head, box_regions, ws, connectivity=8, background=0, min_area=1,
                det_to_seg=None, geom=None, flag=None, fn="seg_regions"):
    """The connected regions of the class map by the rule of `decode.seg_regions_host` (vrnet_seg_regions_u8): class_map
    (B, ihm, iwm) uint8; rows (n_cap >= 1, 5) / offsets (B + 1) int32 as `detect_finish[_ragged]` leave them -> labels
    (B, ihm, iwm) int32, table (B, max_regions, 12) int32 -- the vrnet_region records of `decode.REGION_DTYPE` as words,
    max_regions in [1, 4096] --, head (B, 4) int32 and box_regions (B, cap) int32, every element written; ws: uint8, at least
    seg_regions_workspace_bytes(B, ihm, iwm) bytes; det_to_seg: (n) int32 on the device, one seg class per detection class, or
    None; geom (`_table_call`): the (B, GEOM_BYTES) table of a ragged batch, None: every image fills its slot; flag (1) int32
    or None: FLAG_REGIONS for more regions than max_regions, FLAG_GEOMETRY for a bad record (an image without regions).  Seven
    launches, no host synchronisation."""
    table_call = _table_call(fn, geom)
    if class_map is None or class_map.dim() != 3:
        raise RuntimeError(f"{fn}: expected a contiguous uint8 class map of shape (B, ihm, iwm)")
    B, ihm, iwm = class_map.shape
    if ihm * iwm >= 1 << 31:
        raise RuntimeError(f"{fn}: a slot of {ihm} x {iwm} has 2^31 pixels or more")
    if rows is None or rows.dim() != 2 or rows.shape[0] < 1 or offsets is None or labels is None or head is None or ws is None:
        raise RuntimeError(f"{fn}: rows (n_cap >= 1, 5), offsets, labels, table, head, box_regions and the workspace are required")
    if table is None or table.dim() != 3 or table.shape[1] < 1 or table.shape[2] != REGION_WORDS:
        raise RuntimeError(f"{fn}: expected table ({B}, max_regions, {REGION_WORDS}) int32, the records as words")
    if box_regions is None or box_regions.dim() != 2 or box_regions.shape[1] < 1:
        raise RuntimeError(f"{fn}: expected box_regions ({B}, cap >= 1) int32")
    n_cap, R, cap = rows.shape[0], table.shape[1], box_regions.shape[1]
    n_det = 0 if det_to_seg is None else det_to_seg.numel()
    _tensors(fn, ((class_map, (B, ihm, iwm), torch.uint8), (rows, (n_cap, 5), torch.int32), (offsets, (B + 1,), torch.int32),
                  (labels, (B, ihm, iwm), torch.int32), (table, (B, R, REGION_WORDS), torch.int32),
                  (head, (B, REGION_HEAD), torch.int32), (box_regions, (B, cap), torch.int32), (det_to_seg, (n_det,), torch.int32),
                  (flag, (1,), torch.int32), (ws, (ws.numel(),), torch.uint8)))
    _check(_lib.vrnet_seg_regions_u8(ptr(class_map), B, ihm, iwm, _geom(geom, B, fn) if table_call else None, ihm, iwm, ptr(rows),
                                     ptr(offsets), n_cap, cap, int(connectivity), int(background), int(min_area), R,
                                     ptr(det_to_seg), n_det, ptr(labels), ptr(table), ptr(head), ptr(box_regions), ptr(flag),
                                     ptr(ws), ws.numel(), stream()), fn)
    return labels, table, head, box_regions


# ---- dark-channel dehazing (csrc/dehaze.hip) ---------------------------------------------------------------------------------
FLAG_DEHAZE = 8192       # VR_FLAG_DEHAZE of csrc/common.h: a degenerate image, returned unchanged


def dehaze_workspace_bytes(B, ihm, iwm):
    n = _lib.vrnet_dehaze_workspace_bytes(B, ihm, iwm)
    if n < 0:
        raise RuntimeError(f"dehaze: bad shape (B {B}, slots of {ihm} x {iwm}; 1..65535 images, sides up to 2^17, at most 2^26 "
                           "pixels each and 2^31 in all)")
    return n


def dehaze(frames, out, ws, geom=None, sz=15, r=60, eps=1e-4, omega=0.95, tx=0.1, transmission=None, flag=None):
    """Dark-channel-prior dehazing by the rule of `render.dehaze_host` (vrnet_dehaze_u8): frames (B, ihm, iwm, 3) uint8 ->
    out, another tensor of the same shape; transmission (B, ihm, iwm) float64 or None; ws: uint8, at least
    dehaze_workspace_bytes(B, ihm, iwm) bytes -- its first 32 B bytes hold (A_r, A_g, A_b, degenerate) as float64 per image
    afterwards; geom: the (B, GEOM_BYTES) table of a ragged batch, None: every image fills its slot; flag (1) int32 or
    None: FLAG_DEHAZE for a degenerate image (returned unchanged, t = 1), FLAG_GEOMETRY for a bad record (a zero image).
    Eleven launches, no host synchronisation."""
    fn = "dehaze"
    if frames is None or frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected contiguous uint8 frames of shape (B, ihm, iwm, 3)")
    B, ihm, iwm = frames.shape[:3]
    if out is None or ws is None or out.data_ptr() == frames.data_ptr():
        raise RuntimeError(f"{fn}: out (a tensor other than frames) and the workspace are required")
    _tensors(fn, ((frames, (B, ihm, iwm, 3), torch.uint8), (out, (B, ihm, iwm, 3), torch.uint8),
                  (transmission, (B, ihm, iwm), torch.float64), (flag, (1,), torch.int32), (ws, (ws.numel(),), torch.uint8)))
    _check(_lib.vrnet_dehaze_u8(ptr(frames), None if geom is None else _geom(geom, B, fn), B, ihm, iwm, int(sz), int(r), float(eps),
                                float(omega), float(tx), ptr(out), ptr(transmission), ptr(flag), ptr(ws), ws.numel(), stream()), fn)


# ---- ACE de-rain enhancement (csrc/ace.hip) ------------------------------------------------------------------------------------
FLAG_ACE = 16384         # VR_FLAG_ACE of csrc/common.h: a degenerate image, returned unchanged


def ace_workspace_bytes(B, ihm, iwm):
    n = _lib.vrnet_ace_workspace_bytes(B, ihm, iwm)
    if n < 0:
        raise RuntimeError(f"ace: bad shape (B {B}, slots of {ihm} x {iwm}; 1..65535 images, sides up to 2^17, at most 2^26 "
                           "pixels each and 2^31 in all)")
    return n


def ace(frames, out, ws, weights, geom=None, ratio=4.0, radius=3, s=0.005, bins=2000, flag=None):
    """Automatic Colour Equalisation by the rule of `render.ace_host` (vrnet_ace_u8): frames (B, ihm, iwm, 3) uint8 -> out,
    another tensor of the same shape; ws: uint8, at least ace_workspace_bytes(B, ihm, iwm) bytes; weights: the
    (2 radius + 1, 2 radius + 1) float64 table of `render.ace_weights` on the device; geom: the (B, GEOM_BYTES) table of a
    ragged batch, None: every image fills its slot; flag (1) int32 or None: FLAG_ACE for a degenerate image (returned
    unchanged), FLAG_GEOMETRY for a bad record (a zero image).  2 N + 4 launches for a slot with N pyramid levels above its
    bottom, no host synchronisation."""
    fn = "ace"
    if frames is None or frames.dim() != 4 or frames.shape[-1] != 3:
        raise RuntimeError(f"{fn}: expected contiguous uint8 frames of shape (B, ihm, iwm, 3)")
    B, ihm, iwm = frames.shape[:3]
    if out is None or ws is None or weights is None or out.data_ptr() == frames.data_ptr():
        raise RuntimeError(f"{fn}: out (a tensor other than frames), the weights and the workspace are required")
    n = 2 * int(radius) + 1
    _tensors(fn, ((frames, (B, ihm, iwm, 3), torch.uint8), (out, (B, ihm, iwm, 3), torch.uint8), (weights, (n, n), torch.float64),
                  (flag, (1,), torch.int32), (ws, (ws.numel(),), torch.uint8)))
    _check(_lib.vrnet_ace_u8(ptr(frames), None if geom is None else _geom(geom, B, fn), B, ihm, iwm, int(radius), float(ratio),
                             float(s), int(bins), ptr(weights), ptr(out), ptr(flag), ptr(ws), ws.numel(), stream()), fn)
