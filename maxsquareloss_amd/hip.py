"""ctypes binding of libmsl_hip.so (the C-ABI declared in include/msl_hip.h).

This is the only place the product path reaches native code.  There is no
fallback: if the library is missing or no GPU is visible, every compute call
raises.  `import torch` happens before the library is loaded so that its
libamdhip64.so.7 dependency resolves to the HIP runtime torch already mapped
(one runtime per process, so torch's hipStream_t handles are valid here).
"""
import ctypes
import os

import torch

# MSL_LIB_PATH: another build of the same library (same-box A/B of kernel changes, scripts/bench_ops.py)
LIB_PATH = os.environ.get("MSL_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                          "libmsl_hip.so")

c_int, c_ll, c_sz, c_f, c_p = ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_float, ctypes.c_void_p
c_d = ctypes.c_double

# name -> (restype, argtypes); must match include/msl_hip.h exactly.
SIGNATURES = {
    "msl_abi_version": (c_int, []),
    "msl_status_string": (ctypes.c_char_p, [c_int]),
    "msl_dconv_packed_elems": (c_ll, [c_int, c_int, c_int, c_int]),
    "msl_forms_default": (c_int, [c_p]),
    "msl_forms_check": (c_int, [c_p]),
    "msl_dconv_pack": (c_int, [c_p, c_ll, c_int, c_int, c_int, c_int, c_p, c_p, c_p]),
    "msl_conv_pack_blocks": (c_ll, [c_int] * 5),
    "msl_conv_pack_many": (c_int, [c_p, c_p, c_int, c_int, c_ll, c_p, c_p]),
    "msl_dconv_fwd_workspace": (c_sz, [c_int] * 6),
    "msl_dconv_fwd": (c_int, [c_p, c_p, c_p, c_p] + [c_int] * 8 + [c_p, c_p, c_sz, c_p]),
    "msl_dconv_dgrad_workspace": (c_sz, [c_int] * 6),
    "msl_dconv_dgrad": (c_int, [c_p, c_p, c_p] + [c_int] * 8 + [c_p, c_p, c_sz, c_p]),
    "msl_dconv_wgrad_workspace": (c_sz, [c_int] * 6),
    "msl_dconv_wgrad": (c_int, [c_p, c_p, c_p, c_p] + [c_int] * 9 + [c_p, c_p, c_sz, c_p]),
    "msl_pconv_packed_elems": (c_ll, [c_int] * 3),
    "msl_pconv_pack": (c_int, [c_p, c_int, c_int, c_int, c_p, c_p, c_p]),
    "msl_pconv_fwd_workspace": (c_sz, [c_int] * 3),
    "msl_pconv_fwd": (c_int, [c_p, c_p, c_p] + [c_int] * 3 + [c_p, c_p, c_sz, c_p]),
    "msl_pconv_dgrad_workspace": (c_sz, [c_int] * 3),
    "msl_pconv_dgrad": (c_int, [c_p, c_p, c_p] + [c_int] * 3 + [c_p, c_p, c_sz, c_p]),
    "msl_pconv_dgrad_acc": (c_int, [c_p, c_p, c_p] + [c_int] * 4 + [c_p, c_p, c_sz, c_p]),
    "msl_pconv_wgrad_workspace": (c_sz, [c_int] * 3),
    "msl_pconv_wgrad": (c_int, [c_p, c_p, c_p] + [c_int] * 4 + [c_p, c_p, c_sz, c_p]),
    "msl_absmax_partials": (c_int, [c_p, c_int, c_int, c_p, c_p]),
    "msl_dconv_fwd_sc": (c_int, [c_p, c_p, c_p, c_p] + [c_int] * 8 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_dconv_dgrad_sc": (c_int, [c_p, c_p, c_p] + [c_int] * 8 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_dconv_wgrad_sc": (c_int, [c_p, c_p, c_p, c_p] + [c_int] * 9 + [c_p, c_p, c_sz, c_p, c_p, c_int, c_p, c_int]),
    "msl_pconv_fwd_sc": (c_int, [c_p, c_p, c_p] + [c_int] * 3 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_pconv_dgrad_acc_sc": (c_int, [c_p, c_p, c_p] + [c_int] * 4 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_pconv_wgrad_sc": (c_int, [c_p, c_p, c_p] + [c_int] * 4 + [c_p, c_p, c_sz, c_p, c_p, c_int, c_p, c_int]),
    "msl_dconv_fwd_f16": (c_int, [c_p] * 4 + [c_int] * 8 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_dconv_dgrad_f16": (c_int, [c_p] * 3 + [c_int] * 8 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_dconv_wgrad_f16": (c_int, [c_p] * 4 + [c_int] * 9 + [c_p, c_p, c_sz, c_p, c_p, c_int, c_p, c_int]),
    "msl_pconv_fwd_f16": (c_int, [c_p] * 3 + [c_int] * 3 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_pconv_dgrad_f16": (c_int, [c_p] * 3 + [c_int] * 4 + [c_p, c_p, c_sz, c_p, c_p, c_int]),
    "msl_pconv_wgrad_f16": (c_int, [c_p] * 3 + [c_int] * 4 + [c_p, c_p, c_sz, c_p, c_p, c_int, c_p, c_int]),
    "msl_conv_wgrad_split": (c_int, [c_int] * 7),
    "msl_conv_fwd_form_count": (c_int, []),
    "msl_conv_fwd_form_describe": (c_int, [c_int, c_p]),
    "msl_conv_fwd_plan": (c_int, [c_int] * 8 + [c_p, c_p]),
    "msl_conv_wgrad_plan": (c_int, [c_int] * 11 + [c_p, c_p]),
    "msl_dconv_fwd_bf16": (c_int, [c_p, c_p, c_p, c_p] + [c_int] * 8 + [c_p, c_p, c_sz, c_p]),
    "msl_dconv_dgrad_bf16": (c_int, [c_p, c_p, c_p] + [c_int] * 8 + [c_p, c_p, c_sz, c_p]),
    "msl_dconv_wgrad_bf16": (c_int, [c_p, c_p, c_p, c_p] + [c_int] * 9 + [c_p, c_p, c_sz, c_p]),
    "msl_pconv_fwd_bf16": (c_int, [c_p, c_p, c_p] + [c_int] * 3 + [c_p, c_p, c_sz, c_p]),
    "msl_pconv_dgrad_bf16": (c_int, [c_p, c_p, c_p] + [c_int] * 3 + [c_p, c_p, c_sz, c_p]),
    "msl_pconv_wgrad_bf16": (c_int, [c_p, c_p, c_p] + [c_int] * 4 + [c_p, c_p, c_sz, c_p]),
    "msl_upsample_fwd": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p]),
    "msl_upsample_bwd_workspace": (c_sz, [c_int] * 5),
    "msl_upsample_bwd": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p, c_sz, c_p]),
    "msl_loss_workspace": (c_sz, [c_int] * 5),
    "msl_loss_stats_elems": (c_int, []),
    "msl_ce_up_fwd": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_sz, c_p]),
    "msl_ce_up_bwd": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_maxsquare_up_fwd": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_sz, c_p]),
    "msl_maxsquare_up_bwd": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_iw_maxsquare_up_fwd": (c_int, [c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_iw_maxsquare_up_bwd": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_multi_ce_up_fwd": (c_int, [c_p, c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p, c_sz, c_p]),
    "msl_multi_ce_up_bwd": (c_int, [c_p, c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_loss_labels_up": (c_int, [c_p, c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p]),
    "msl_entropy_up_fwd": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_sz, c_p]),
    "msl_entropy_up_bwd": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_iw_entropy_up_fwd": (c_int, [c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_iw_entropy_up_bwd": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_hard_ce_up_fwd": (c_int, [c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p, c_sz, c_p]),
    "msl_hard_ce_up_bwd": (c_int, [c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_pseudo_labels_up": (c_int, [c_p] + [c_int] * 5 + [c_f, c_p, c_p, c_p]),
    "msl_soft_ce_fwd": (c_int, [c_p, c_p, c_int, c_int, c_f, c_p, c_p, c_p, c_sz, c_p]),
    "msl_soft_ce_bwd": (c_int, [c_p, c_p, c_int, c_int, c_f, c_p, c_p, c_p, c_p, c_p]),
    "msl_iw_soft_ce_fwd": (c_int, [c_p, c_p, c_int, c_int, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_iw_soft_ce_bwd": (c_int, [c_p, c_p, c_int, c_int, c_f, c_p, c_p, c_p, c_p, c_p]),
    "msl_maxsquare_prob_fwd": (c_int, [c_p, c_int, c_int, c_p, c_p, c_sz, c_p]),
    "msl_maxsquare_prob_bwd": (c_int, [c_p, c_int, c_int, c_p, c_p, c_p]),
    "msl_iw_maxsquare_prob_fwd": (c_int, [c_p, c_p, c_int, c_int, c_f, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_iw_maxsquare_prob_bwd": (c_int, [c_p, c_int, c_int, c_p, c_p, c_p, c_p]),
    "msl_confusion_accumulate": (c_int, [c_p, c_p, c_int, ctypes.c_longlong, c_p, c_p, c_p]),
    "msl_predict_up": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_p]),
    "msl_predict_images": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p, c_p, c_f] + [c_p] * 9),
    "msl_colorize": (c_int, [c_p, c_int, c_ll, c_p, c_int, c_p, c_p]),
    "msl_bn_uses_fused": (c_int, [c_int, c_int, c_int, c_p]),
    "msl_bn_workspace": (c_sz, [c_int] * 3),
    "msl_bn_fwd": (c_int, [c_p] * 10 + [c_int] * 5 + [c_f, c_f, c_int, c_p, c_p, c_sz, c_p]),
    "msl_bn_bwd": (c_int, [c_p] * 10 + [c_int] * 6 + [c_p, c_p, c_sz, c_p]),
    "msl_bn_fwd_am": (c_int, [c_p] * 10 + [c_int] * 5 + [c_f, c_f, c_int, c_p, c_p, c_sz, c_p, c_p]),
    "msl_bn_bwd_am": (c_int, [c_p] * 10 + [c_int] * 6 + [c_p, c_p, c_sz, c_p, c_p]),
    "msl_bn_bwd_am_beta": (c_int, [c_p] * 11 + [c_int] * 6 + [c_p, c_p, c_sz, c_p, c_p]),
    "msl_bn_relu_mask_bytes": (c_sz, [c_int] * 3),
    "msl_bn_fwd_mask": (c_int, [c_p] * 10 + [c_int] * 5 + [c_f, c_f, c_int, c_p, c_p, c_sz, c_p, c_p, c_p]),
    "msl_bn_bwd_mask": (c_int, [c_p] * 11 + [c_int] * 6 + [c_p, c_p, c_sz, c_p, c_p]),
    "msl_bn_plan": (c_int, [c_int] * 12 + [c_sz, c_p, c_p]),
    "msl_loss_plan": (c_int, [c_int] * 6 + [c_sz, c_p]),
    "msl_image_transform": (c_int, [c_p, c_int, c_int, c_int, c_f, c_f, c_f, c_p, c_p]),
    "msl_label_transform": (c_int, [c_p, c_int, c_int, c_int, c_p, c_p, c_p]),
    "msl_resize_workspace": (c_sz, [c_int, c_int]),
    "msl_resize_bicubic_rgb": (c_int, [c_p] + [c_int] * 7 + [c_p, c_p, c_int, c_p, c_p, c_int, c_int, c_int, c_p, c_p,
                                       c_f, c_f, c_f, c_p, c_sz, c_p]),
    "msl_resize_nearest_label": (c_int, [c_p] + [c_int] * 7 + [c_p, c_p, c_int, c_int, c_p, c_p, c_p, c_p]),
    "msl_png_unfilter_lane": (c_int, [c_p, c_int, c_int, c_int, c_int, c_sz, c_p, c_p]),
    "msl_png_unfilter_band_rows": (c_int, []),
    "msl_jpeg_info": (c_int, [c_p, c_sz, c_p]),
    "msl_jpeg_coef_elems": (c_sz, [c_p]),
    "msl_jpeg_entropy_decode": (c_int, [c_p, c_sz, c_p, c_p, c_sz, c_p]),
    "msl_jpeg_workspace": (c_sz, [c_p]),
    "msl_jpeg_reconstruct": (c_int, [c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "msl_jpeg_tile_blocks": (c_int, []),
    "msl_jpeg_tile_pixels": (c_int, []),
    "msl_im2col": (c_int, [c_p] + [c_int] * 11 + [c_p, c_p]),
    "msl_col2im": (c_int, [c_p] + [c_int] * 11 + [c_p, c_p]),
    "msl_maxpool_fwd": (c_int, [c_p] + [c_int] * 8 + [c_p, c_p, c_p]),
    "msl_maxpool_bwd": (c_int, [c_p, c_p] + [c_int] * 8 + [c_p, c_p]),
    "msl_subsample": (c_int, [c_p] + [c_int] * 6 + [c_p, c_p]),
    "msl_subsample_bwd": (c_int, [c_p] + [c_int] * 6 + [c_p, c_p]),
    "msl_aspp_weight_layout": (c_int, [c_p, c_ll, c_int, c_int, c_int, c_p, c_p]),
    "msl_aspp_weight_grad": (c_int, [c_p, c_int, c_int, c_int, c_p, c_p]),
    "msl_aspp_shift_add": (c_int, [c_p, c_p, c_p] + [c_int] * 7 + [c_p]),
    "msl_aspp_shift_gather": (c_int, [c_p, c_p, c_p] + [c_int] * 7 + [c_p]),
    "msl_sgd_block_elems": (c_int, []),
    "msl_sgd_plan": (c_ll, [c_p, c_int, c_p, c_p, c_ll]),
    "msl_sgd_step": (c_int, [c_p, c_p, c_p, c_ll, c_f, c_f, c_f, c_f, c_f, c_p]),
    "msl_sgd_step_lr_dev": (c_int, [c_p, c_p, c_p, c_ll, c_p, c_f, c_f, c_f, c_p]),
    "msl_adam_max_mult": (c_int, []),
    "msl_adam_coef_bytes": (c_sz, [c_int]),
    "msl_adam_step": (c_int, [c_p, c_int, c_p, c_p, c_ll, c_f, c_f, c_d, c_d, c_d, c_f, c_f, c_p, c_p]),
    "msl_adam_step_lr_dev": (c_int, [c_p, c_int, c_p, c_p, c_ll, c_p, c_d, c_d, c_d, c_f, c_f, c_p, c_p]),
    "msl_style_pad": (c_int, [c_p] + [c_int] * 6 + [c_p, c_p, c_p, c_int, c_p]),
    "msl_style_input": (c_int, [c_p, c_p, c_int, c_int, c_p, c_p, c_p, c_int, c_p]),
    "msl_style_stats_workspace": (c_sz, [c_int] * 3),
    "msl_style_stats": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p, c_sz, c_p]),
    "msl_style_max_styles": (c_int, []),
    "msl_style_adain_coef": (c_int, [c_p, c_p, c_p, c_int, c_int, c_f, c_f, c_p, c_p, c_p]),
    "msl_style_output": (c_int, [c_p] + [c_int] * 3 + [c_p, c_p, c_f, c_f, c_f, c_p]),
    "msl_style_input_window": (c_int, [c_p, c_p] + [c_int] * 8 + [c_p, c_p, c_p, c_int, c_p]),
    "msl_style_output_resampled": (c_int, [c_p] + [c_int] * 9 + [c_p] + [c_int] * 6 + [c_f, c_f, c_f, c_p]),
    "msl_label_resize_nearest": (c_int, [c_p, c_int, c_int, c_p, c_int, c_int, c_p]),
    "msl_predict_rectify": (c_int, [c_p, c_p, c_p] + [c_int] * 6 + [c_p, c_p, c_p, c_p]),
    "msl_resize_bilinear": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p]),
    "msl_predict_tta_max_entries": (c_int, []),
    "msl_predict_tta": (c_int, [c_p] + [c_int] * 4 + [c_p, c_p, c_p, c_p]),
    "msl_predict_tta_images": (c_int, [c_p] + [c_int] * 4 + [c_p, c_p, c_f] + [c_p] * 9),
    "msl_confidence_hist": (c_int, [c_p, c_p] + [c_int] * 6 + [c_p, c_p]),
    "msl_confidence_hist_tta": (c_int, [c_p] + [c_int] * 5 + [c_p, c_p]),
    "msl_class_thresholds": (c_int, [c_p, c_int, c_int, c_d, c_f, c_p, c_p, c_p]),
    "msl_pseudo_classwise": (c_int, [c_p, c_p] + [c_int] * 5 + [c_p, c_p, c_p, c_p]),
    "msl_pseudo_classwise_tta": (c_int, [c_p] + [c_int] * 4 + [c_p, c_p, c_p, c_p]),
    "msl_image_metrics": (c_int, [c_p, c_p, c_int, c_d, c_p, c_int, c_p, c_p]),
    "msl_analysis_maps": (c_int, [c_p] * 5 + [c_int] * 3 + [c_p, c_ll] + [c_p] * 5),
    "msl_launch_guard_probe": (c_int, [c_int, c_p, c_p]),
    "msl_pconv_dgrad_resmask_sc": (c_int, [c_p, c_p, c_p, c_int, c_int, c_int, c_p, c_p, c_int, c_p, c_p, c_sz, c_p, c_p,
                                           c_int]),
    "msl_pconv_dgrad_resmask_f16": (c_int, [c_p, c_p, c_p, c_int, c_int, c_int, c_p, c_p, c_int, c_p, c_p, c_sz, c_p,
                                            c_p, c_int]),
}

ABI_VERSION = 3
# r06 entry points an older build (MSL_LIB_PATH, a same-box A/B) may lack: the diagnostics probe and the masked
# residual dgrad (ops.py falls back to the materialised residual gradient without it)
# and the prediction-image entry points (ops.predict_images / ops.colorize raise without them), as do the
# per-image analysis ones (ops.image_metrics / ops.analysis_maps) and the class-threshold ones
# (ops.confidence_hist / ops.class_thresholds / ops.pseudo_classwise)
_DIAGNOSTIC = {"msl_launch_guard_probe", "msl_pconv_dgrad_resmask_sc", "msl_pconv_dgrad_resmask_f16",
               "msl_predict_images", "msl_colorize", "msl_image_metrics", "msl_analysis_maps",
               "msl_confidence_hist", "msl_confidence_hist_tta", "msl_class_thresholds", "msl_pseudo_classwise",
               "msl_pseudo_classwise_tta"}
_lib = None


class MSLError(RuntimeError):
    pass


_gpu_seen = False


def load(require_gpu=True):
    """Load libmsl_hip.so and declare every C-ABI symbol.  Raises if absent."""
    global _lib, _gpu_seen
    if require_gpu and not _gpu_seen:
        if not torch.cuda.is_available():
            raise MSLError("maxsquareloss_amd: no GPU visible; the HIP path has no CPU fallback")
        _gpu_seen = True  # a visible GPU stays visible: skip the per-op query
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MSLError(f"maxsquareloss_amd: {LIB_PATH} is missing; run __graft_entry__.build() "
                       "(make -C maxsquareloss_amd/csrc)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if name in _DIAGNOSTIC and not hasattr(lib, name):
            continue  # an older build (MSL_LIB_PATH, a same-box A/B) without the diagnostics entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.msl_abi_version() != ABI_VERSION:
        raise MSLError("libmsl_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load(require_gpu=False).msl_status_string(status).decode()
        raise MSLError(f"{what} failed: {msg} (status {status})")


def stream_ptr():
    """torch's current HIP stream on the current device, as the raw hipStream_t every entry point
    takes (the direct accessor: torch.cuda.current_stream() costs ~8 us of Python per op)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def ptr(t):
    return None if t is None else t.data_ptr()


class Forms(ctypes.Structure):
    """msl_forms (include/msl_hip.h): the kernel forms every conv / pack / BN call takes (ABI 3)."""
    _fields_ = [("f32_form", c_int), ("sk_hybrid", c_int), ("pack_form", c_int), ("bn_fused", c_int)]


class TtaEntry(ctypes.Structure):
    """msl_tta_entry: one low-resolution prediction of msl_predict_tta / msl_predict_tta_images."""
    _fields_ = [("logits", c_p), ("hi", c_int), ("wi", c_int), ("mirror", c_int)]


class JpegComp(ctypes.Structure):
    """msl_jpeg_comp: one component of a msl_jpeg_header."""
    _fields_ = [(n, ctypes.c_int32) for n in ("h", "v", "tq", "blocks_w", "blocks_h", "reserved")] + [
        ("offset", ctypes.c_int64)]


class JpegHeader(ctypes.Structure):
    """msl_jpeg_header: what msl_jpeg_info / msl_jpeg_entropy_decode say about a file (utils/jpeg.py)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "ncomp", "hmax", "vmax", "restart_interval",
                                              "mcus_w", "mcus_h")] + [("comp", JpegComp * 3)]


class ConvForm(ctypes.Structure):
    """msl_conv_form: one instantiation of the stream-K forward-form kernel (msl_conv_fwd_form_describe)."""
    _fields_ = [(n, c_int) for n in ("bm", "G", "stages", "wm", "wn", "pw", "math", "acc", "bform")]


class ConvFwdPlan(ctypes.Structure):
    """msl_conv_fwd_plan_info: the plan of one forward-form call (msl_conv_fwd_plan; host only)."""
    _fields_ = [(n, c_int) for n in ("row", "stream_k", "math", "tiles_m", "tiles_n", "ksteps", "kps", "S", "tdp",
                                     "NW", "T", "reduce", "split_img", "status")]


def conv_fwd_plan(family, nbranch, taps, cimg, m, p, accumulate, dil0, forms_=None):
    """The plan of a forward-form call as a ConvFwdPlan (no GPU needed); `forms_` defaults to FORMS."""
    out = ConvFwdPlan()
    fm = forms() if forms_ is None else ctypes.addressof(forms_)
    check(load(require_gpu=False).msl_conv_fwd_plan(family, nbranch, taps, cimg, m, p, accumulate, dil0, fm,
                                                    ctypes.addressof(out)), "msl_conv_fwd_plan")
    return out


class ConvWgradPlan(ctypes.Structure):
    """msl_conv_wgrad_plan_info: the plan of one weight-gradient call (msl_conv_wgrad_plan; host only)."""
    _fields_ = [(n, c_int) for n in ("gemm", "bm", "bn", "math", "split_rows", "reduce", "trans", "tiles_m", "tiles_n",
                                     "ntap", "KS", "bk", "NW", "T", "slots", "nchunk", "kchunk", "swizzle", "max_run",
                                     "mask_tab", "rowscale", "status")]


def conv_wgrad_plan(family, nbranch, taps, cin, cout, h, w, nimg, has_dbias=0, x_npart=0, dy_npart=0, forms_=None):
    """The plan of a weight-gradient call as a ConvWgradPlan (no GPU needed); `forms_` defaults to FORMS."""
    out = ConvWgradPlan()
    fm = forms() if forms_ is None else ctypes.addressof(forms_)
    check(load(require_gpu=False).msl_conv_wgrad_plan(family, nbranch, taps, cin, cout, h, w, nimg, has_dbias, x_npart,
                                                      dy_npart, fm, ctypes.addressof(out)), "msl_conv_wgrad_plan")
    return out


class BnPlan(ctypes.Structure):
    """msl_bn_plan_info: the plan of one BN call (msl_bn_plan; host only)."""
    _fields_ = [(n, c_int) for n in ("status", "fused", "ept", "joint", "vec", "S", "chunk", "max_rows", "launches")] + [
        ("grid_x", c_int * 2), ("grid_y", c_int * 2), ("block", c_int * 2)]


BN_RELU_SOURCES = {"none": 0, "y": 1, "bits": 2, "recompute": 3}
BN_BWD_ENTRIES = {"am": 0, "am_beta": 1, "mask": 2}


def bn_plan(backward, c, p, nimg, training, relu, aligned=1, entry="am", relu_src="none", has_dx=0, has_absmax=0,
            has_mask=0, ws_bytes=None, forms_=None):
    """The plan of a BN call as a BnPlan (no GPU needed); `forms_` defaults to FORMS, `ws_bytes` to what
    msl_bn_workspace asks.  The call's own refusal is in .status; arguments that describe no call raise."""
    lib = load(require_gpu=False)
    out = BnPlan()
    fm = forms() if forms_ is None else ctypes.addressof(forms_)
    if ws_bytes is None:
        ws_bytes = lib.msl_bn_workspace(c, p, nimg)
    check(lib.msl_bn_plan(int(backward), c, p, nimg, int(training), int(relu), int(aligned), BN_BWD_ENTRIES[entry],
                          BN_RELU_SOURCES[relu_src], int(has_dx), int(has_absmax), int(has_mask), ws_bytes, fm,
                          ctypes.addressof(out)), "msl_bn_plan")
    return out


class LossPlan(ctypes.Structure):
    """msl_loss_plan_info: the plan of one fused-loss / upsample / resize call (msl_loss_plan; host only)."""
    _fields_ = [(n, c_int) for n in ("status", "cm", "fwd_blocks", "fwd_trips", "rows_chunks", "per", "rows_wmax",
                                     "lds_optin", "cols_blocks", "cols_trips", "vec", "four_tap")] + [
        ("lds_bytes", c_ll), ("ws_required", c_ll)]


LOSS_FAMILIES = {"up_fwd": 0, "up_bwd": 1, "upsample_bwd": 2, "upsample_fwd": 3, "resize": 4, "prob_fwd": 5,
                 "prob_bwd": 6, "soft_fwd": 7, "soft_bwd": 8, "labels": 9}


def loss_plan(family, c, hi, wi, ho, wo, ws_bytes=None):
    """The plan of a call of `family` (LOSS_FAMILIES) as a LossPlan (no GPU needed); the flat families take
    ho * wo pixels.  `ws_bytes` defaults to what msl_loss_workspace asks (for msl_upsample_bwd, what
    msl_upsample_bwd_workspace asks).  The call's own refusal is in .status."""
    lib = load(require_gpu=False)
    out = LossPlan()
    if ws_bytes is None:
        if family == "upsample_bwd":
            ws_bytes = lib.msl_upsample_bwd_workspace(c, hi, wi, ho, wo) if min(c, hi, wi, ho, wo) >= 1 else 0
        elif family.startswith(("prob", "soft")):
            ws_bytes = lib.msl_loss_workspace(c, 1, 1, 1, ho * wo)
        else:
            ws_bytes = lib.msl_loss_workspace(c, hi, wi, ho, wo)
    check(lib.msl_loss_plan(LOSS_FAMILIES[family], c, hi, wi, ho, wo, ws_bytes, ctypes.addressof(out)),
          "msl_loss_plan")
    return out


FORMS = Forms(5, 1, 1, 1)  # the forms this process passes: the library's defaults until set_form


def forms():
    """The const msl_forms* of every conv / pack / BN call: FORMS, read by the library on the host when
    the call launches (a captured graph keeps the forms of its capture)."""
    return ctypes.addressof(FORMS)


def snapshot_forms():
    """A copy of FORMS: an autograd function keeps the forms of its forward and passes them to
    its backward's calls, so a form switched between the two (the tests toggle them) cannot hand a
    backward kernel a state its forward did not leave (the fused BN's mask bits, a pack's form)."""
    return Forms(*(getattr(FORMS, f) for f, _ in Forms._fields_))


def set_form(name, value):
    """Set one field of FORMS (checked by msl_forms_check); returns the previous value."""
    trial = Forms(*(getattr(FORMS, f) for f, _ in Forms._fields_))
    setattr(trial, name, int(value))
    check(load(require_gpu=False).msl_forms_check(ctypes.addressof(trial)), f"msl_forms {name}={value}")
    prev = getattr(FORMS, name)
    setattr(FORMS, name, int(value))
    return prev


def workspace(nbytes, device):
    """Scratch from the caching allocator (stream-ordered reuse, no sync)."""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
