"""ctypes binding of libuaps_hip.so (C ABI: include/uaps_hip.h).

There is no fallback: if the shared library is missing or a symbol is absent, every op that needs it
raises.  `python -c "import __graft_entry__ as g; g.build()"` (or `make -C uaps_amd/csrc`) builds it.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

from . import config

_HERE = os.path.dirname(os.path.abspath(__file__))
# UAPS_HIP_LIB selects another build of the same ABI (tools/ab_bench.sh compares two kernel builds on one GPU box)
LIB_PATH = config.text("UAPS_HIP_LIB") or os.path.join(_HERE, "lib", "libuaps_hip.so")
CSRC = os.path.join(_HERE, "csrc")

_lock = threading.Lock()
_tls = threading.local()      # one reusable uaps_call_hints ARGUMENT buffer per Python thread (the *_h entry points copy it during the call)
_lib = None

c_float_p = C.POINTER(C.c_float)
c_void_p = C.c_void_p

# symbol -> (restype, argtypes); mirrors include/uaps_hip.h one to one
_PTR = C.c_void_p
SIGNATURES = {
    "uaps_abi_version": (C.c_int, []),
    "uaps_error_string": (C.c_char_p, [C.c_int]),
    "uaps_loss_workspace_bytes": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_size_t)]),
    "uaps_unsup_fwd": (C.c_int, [_PTR, _PTR] + [C.c_int] * 5 + [C.c_float] * 3 + [_PTR, _PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_unsup_bwd": (C.c_int, [_PTR, _PTR, _PTR, C.c_float, C.c_float, _PTR] + [C.c_int] * 5 + [_PTR, _PTR]),
    "uaps_sup_fwd": (C.c_int, [_PTR, _PTR] + [C.c_int] * 5 + [C.c_float] * 3 + [_PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_sup_bwd": (C.c_int, [_PTR, _PTR, _PTR, C.c_float, C.c_float, _PTR] + [C.c_int] * 5 + [_PTR, _PTR]),
    "uaps_pairloss_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "uaps_pairloss_num_sums": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "uaps_pairloss_fwd": (C.c_int, [_PTR] * 4 + [C.c_int] * 5 + [C.c_float] * 3 + [_PTR] * 6 + [C.c_size_t, C.c_int, _PTR]),
    "uaps_pairloss_finalize_sums": (C.c_int, [_PTR, C.c_int, C.c_int, C.c_long] + [C.c_float] * 3 + [_PTR] * 3),
    "uaps_pairloss_bwd": (C.c_int, [_PTR] * 6 + [C.c_float] * 2 + [_PTR] + [C.c_int] * 5 + [C.c_long, _PTR, _PTR, C.c_int, _PTR]),
    "uaps_feat_noise": (C.c_int, [_PTR, _PTR] + [C.c_int] * 4 + [C.c_uint64, C.c_uint64, C.c_float, _PTR, _PTR]),
    "uaps_feat_noise_apply": (C.c_int, [_PTR, _PTR, _PTR, C.c_int, C.c_long, _PTR]),
    "uaps_feat_bernoulli": (C.c_int, [_PTR, _PTR, C.c_long, C.c_uint64, C.c_uint64, C.c_float, _PTR, _PTR]),
    "uaps_feat_mask_apply": (C.c_int, [_PTR, _PTR, C.c_float, _PTR, C.c_long, _PTR]),
    "uaps_feat_dropout_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_feat_dropout_fwd": (C.c_int, [_PTR, _PTR] + [C.c_int] * 4 + [C.c_float, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_feat_dropout_bwd": (C.c_int, [_PTR, _PTR, _PTR] + [C.c_int] * 4 + [_PTR]),
    "uaps_bn_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_bn_act_fwd_train": (C.c_int, [_PTR] * 7 + [C.c_float] * 4 + [C.c_uint64, C.c_uint64] + [C.c_int] * 4 + [_PTR, _PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_bn_act_fwd_train_grouped": (C.c_int, [_PTR] * 7 + [C.c_float] * 4 + [C.c_uint64, C.c_uint64] + [C.c_int] * 5 + [_PTR, _PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_bn_act_fwd_train_partials": (C.c_int, [_PTR, C.c_int] + [_PTR] * 7 + [C.c_float] * 4 + [C.c_uint64, C.c_uint64] + [C.c_int] * 5 + [_PTR, _PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_bn_act_bwd_grouped": (C.c_int, [_PTR] * 6 + [C.c_float] * 2 + [C.c_uint64, C.c_uint64] + [C.c_int] * 5 + [_PTR, _PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_bn_act_bwd_grouped_bias": (C.c_int, [_PTR] * 6 + [C.c_float] * 2 + [C.c_uint64, C.c_uint64] + [C.c_int] * 5 + [_PTR] * 5 + [C.c_size_t, _PTR]),
    "uaps_bn_act_fwd_eval": (C.c_int, [_PTR] * 6 + [C.c_float] * 2 + [C.c_int] * 4 + [_PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_bn_act_bwd": (C.c_int, [_PTR] * 6 + [C.c_float] * 2 + [C.c_uint64, C.c_uint64] + [C.c_int] * 4 + [_PTR, _PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_bn_act_bwd_eval": (C.c_int, [_PTR] * 6 + [C.c_float] * 2 + [C.c_int] * 4 + [_PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_up_cat_fwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 5 + [_PTR]),
    "uaps_up_cat_bwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 5 + [_PTR]),
    "uaps_conv_set_mode": (C.c_int, [C.c_int]),
    "uaps_conv_get_mode": (C.c_int, []),
    "uaps_conv_set_tuning": (C.c_int, [C.c_uint]),
    "uaps_conv_get_tuning": (C.c_uint, []),
    "uaps_set_error_word": (C.c_int, [_PTR]),
    "uaps_conv_pack_floats": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "uaps_conv_pack_weights": (C.c_int, [_PTR] + [C.c_int] * 3 + [_PTR, _PTR, _PTR]),
    "uaps_conv_pack_weights_batch": (C.c_int, [_PTR] * 6 + [C.c_int, _PTR]),
    "uaps_conv_fwd": (C.c_int, [_PTR] * 4 + [C.c_int] * 7 + [_PTR]),
    "uaps_conv_fwd_stats": (C.c_int, [_PTR] * 5 + [C.c_int] * 7 + [_PTR]),
    "uaps_conv_fwd_stats_parts": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_int)]),
    "uaps_conv_bwd_data": (C.c_int, [_PTR] * 3 + [C.c_int] * 7 + [_PTR]),
    "uaps_conv_wrw_workspace_bytes": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_size_t)]),
    "uaps_conv_bwd_weight_partial": (C.c_int, [_PTR, _PTR] + [C.c_int] * 8 + [_PTR, C.c_size_t, _PTR]),
    "uaps_conv_bwd_weight_reduce": (C.c_int, [_PTR, _PTR, _PTR] + [C.c_int] * 7 + [_PTR]),
    "uaps_conv_bwd_weight_reduce_batch": (C.c_int, [_PTR, C.c_int, _PTR]),
    "uaps_conv_fwd_cat": (C.c_int, [_PTR, C.c_int, _PTR, C.c_int] + [_PTR] * 4 + [C.c_int] * 6 + [_PTR]),
    "uaps_conv_bwd_data_cat": (C.c_int, [_PTR, _PTR, _PTR, C.c_int, _PTR, C.c_int] + [C.c_int] * 6 + [_PTR]),
    "uaps_conv_bwd_weight_partial_cat": (C.c_int, [_PTR, _PTR, C.c_int, _PTR, C.c_int] + [C.c_int] * 7 + [_PTR, C.c_size_t, _PTR]),
    "uaps_bn_finalize_train": (C.c_int, [_PTR, C.c_int] + [_PTR] * 6 + [C.c_float] * 2 + [C.c_int] * 5 + [_PTR] * 4),
    "uaps_conv_fwd_bn": (C.c_int, [_PTR, _PTR, C.c_float, C.c_int] + [_PTR] * 4 + [C.c_int] * 7 + [_PTR]),
    "uaps_conv_bwd_weight_partial_bn": (C.c_int, [_PTR, _PTR, _PTR, C.c_float, C.c_int] + [C.c_int] * 8 + [_PTR, C.c_size_t, _PTR]),
    "uaps_conv_fwd_variant": (C.c_int, [C.c_int] * 7 + [C.c_char_p, C.c_size_t]),
    "uaps_conv_wrw_variant": (C.c_int, [C.c_int] * 7 + [C.c_char_p, C.c_size_t]),
    "uaps_conv_bwd_weight": (C.c_int, [_PTR] * 4 + [C.c_int] * 7 + [_PTR, C.c_size_t, _PTR]),
    "uaps_set_step_state": (C.c_int, [_PTR]),
    "uaps_next_call_hints": (C.c_int, [_PTR]),
    "uaps_conv_ex": (C.c_int, [_PTR]),
    "uaps_conv_ex_variant": (C.c_int, [_PTR, C.c_char_p, C.c_size_t]),
    "uaps_account": (C.c_int, [C.c_int]),
    "uaps_accounted_bytes": (C.c_double, []),
    "uaps_next_launch_events": (C.c_int, [_PTR, _PTR]),
    "uaps_zero_bounds": (C.c_int, [_PTR, C.c_long, _PTR]),
    "uaps_bn_param_bounds": (C.c_int, [_PTR, _PTR, _PTR, C.c_int, _PTR, _PTR]),
    "uaps_get_step_state": (C.c_void_p, []),
    "uaps_convs_pack_floats": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "uaps_convs_pack_weights": (C.c_int, [_PTR] + [C.c_int] * 3 + [_PTR, _PTR, _PTR]),
    "uaps_convs_out_size": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "uaps_convs_fwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 8 + [_PTR]),
    "uaps_convs_bwd_data": (C.c_int, [_PTR] * 3 + [C.c_int] * 8 + [_PTR]),
    "uaps_convs_wrw_workspace_bytes": (C.c_int, [C.c_int] * 8 + [C.POINTER(C.c_size_t)]),
    "uaps_convs_bwd_weight": (C.c_int, [_PTR] * 3 + [C.c_int] * 8 + [_PTR, C.c_size_t, _PTR]),
    "uaps_maxpool3x3s2_fwd": (C.c_int, [_PTR, _PTR, _PTR, C.c_long, C.c_int, C.c_int, _PTR]),
    "uaps_maxpool3x3s2_bwd": (C.c_int, [_PTR, _PTR, _PTR, C.c_long, C.c_int, C.c_int, _PTR]),
    "uaps_space_to_depth2": (C.c_int, [_PTR, _PTR, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _PTR]),
    "uaps_subsample2_fwd": (C.c_int, [_PTR, _PTR, C.c_long, C.c_int, C.c_int, _PTR]),
    "uaps_subsample2_bwd": (C.c_int, [_PTR, _PTR, C.c_long, C.c_int, C.c_int, _PTR]),
    "uaps_sum_tensors": (C.c_int, [_PTR, C.c_int, _PTR, C.c_long, _PTR]),
    "uaps_pair_workspace_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
    "uaps_feat_dropout_stats": (C.c_int, [_PTR] + [C.c_int] * 4 + [_PTR, C.c_size_t, _PTR]),
    "uaps_fanout_perturbed": (C.c_int, [_PTR] * 7 + [C.c_int, C.c_int, C.c_uint64, C.c_float, C.c_float] + [C.c_int] * 4 + [_PTR]),
    "uaps_augment_batch": (C.c_int, [_PTR] * 5 + [C.c_uint64] + [C.c_int] * 5 + [C.POINTER(C.c_float), C.POINTER(C.c_float), _PTR, _PTR, _PTR]),
    "uaps_augment_views_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_augment_views": (C.c_int, [_PTR]),
    "uaps_softmax_klmap_bwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 4 + [_PTR] * 3),
    "uaps_softmax_pair_fwd": (C.c_int, [_PTR, _PTR] + [C.c_int] * 5 + [_PTR, _PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_softmax_mse_bwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 4 + [_PTR, _PTR]),
    "uaps_softmax_kl_bwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 4 + [_PTR, _PTR]),
    "uaps_entropy_map": (C.c_int, [_PTR] + [C.c_int] * 4 + [_PTR, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_fanin_perturbed": (C.c_int, [_PTR] * 4 + [C.c_int, C.c_int, C.c_uint64, C.c_float, C.c_float] + [C.c_int] * 4 + [_PTR, _PTR]),
    "uaps_maxpool2x2_fwd": (C.c_int, [_PTR] + [C.c_int] * 4 + [_PTR, _PTR, _PTR]),
    "uaps_adam_step": (C.c_int, [_PTR] * 5 + [C.c_int] + [C.c_double] * 5 + [C.c_long, _PTR]),
    "uaps_add_relu": (C.c_int, [_PTR, _PTR, _PTR, C.c_long, _PTR]),
    "uaps_relu_bwd": (C.c_int, [_PTR, _PTR, _PTR, C.c_long, _PTR]),
    "uaps_relu_bwd_sum": (C.c_int, [_PTR, C.c_int, _PTR, _PTR, C.c_long, _PTR]),
    "uaps_cat2": (C.c_int, [_PTR, _PTR, _PTR, C.c_long, _PTR]),
    "uaps_bn_act_bwd_prepare": (C.c_int, [_PTR] * 6 + [C.c_float] + [C.c_int] * 5 + [_PTR] * 6 + [C.c_size_t, _PTR]),
    "uaps_bn_act_bwd_apply": (C.c_int, [_PTR] * 3 + [C.c_float] + [C.c_int] * 5 + [_PTR, _PTR]),
    "uaps_bn_act_bwd_finalize": (C.c_int, [_PTR, C.c_int] + [_PTR] * 5 + [C.c_int] * 5 + [_PTR] * 6),
    "uaps_head_bwd_fused": (C.c_int, [_PTR] * 3 + [C.c_float, C.c_int, _PTR, _PTR, C.c_float, _PTR, C.c_float] + [_PTR] * 4 + [C.c_int] * 8 +
                            [_PTR] * 4 + [C.c_size_t, _PTR]),
    "uaps_mid_bwd_fused": (C.c_int, [_PTR] * 3 + [C.c_float, C.c_int, _PTR, _PTR, C.c_float, C.c_int, _PTR, _PTR, C.c_float, _PTR, C.c_float] +
                           [_PTR] * 4 + [C.c_int] * 8 + [_PTR] * 4 + [C.c_size_t, _PTR]),
    "uaps_up_bwd_fused": (C.c_int, [_PTR, _PTR, _PTR, C.c_float, _PTR, C.c_int, _PTR] + [C.c_int] * 7 + [_PTR]),
    "uaps_up_fold_support": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "uaps_up_bwd_fused_form": (C.c_int, [C.c_int, C.c_int]),
    "uaps_up_bwd_fused_grid": (C.c_int, [C.c_int, C.c_int]),
    "uaps_seg_confusion": (C.c_int, [_PTR, _PTR] + [C.c_int] * 4 + [_PTR, _PTR]),
    "uaps_ema_update": (C.c_int, [_PTR] * 3 + [C.c_int, C.c_float, C.c_float, _PTR]),
    "uaps_teacher_noise": (C.c_int, [_PTR] + [C.c_int] * 5 + [C.c_uint64, C.c_uint64, _PTR, _PTR]),
    "uaps_teacher_noise_apply": (C.c_int, [_PTR, _PTR] + [C.c_int] * 5 + [_PTR, _PTR]),
    "uaps_mc_consistency_workspace_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
    "uaps_mc_consistency_fwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 5 + [C.c_float] + [_PTR] * 4 + [C.c_size_t, _PTR]),
    "uaps_mc_consistency_bwd": (C.c_int, [_PTR] * 5 + [C.c_int] * 4 + [_PTR, _PTR]),
    "uaps_cct_dct_workspace_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
    "uaps_cct_consistency_fwd": (C.c_int, [_PTR] + [C.c_int] * 6 + [_PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_cct_consistency_bwd": (C.c_int, [_PTR] + [C.c_int] * 6 + [_PTR, _PTR, _PTR]),
    "uaps_rot90_batch": (C.c_int, [_PTR, _PTR] + [C.c_int] * 5 + [_PTR, _PTR, _PTR]),
    "uaps_rot_consistency_fwd": (C.c_int, [_PTR, C.c_int, _PTR] + [C.c_int] * 6 + [_PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_rot_consistency_bwd": (C.c_int, [_PTR, C.c_int, _PTR] + [C.c_int] * 6 + [_PTR, _PTR, _PTR, _PTR]),
    "uaps_cps_workspace_bytes": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_size_t)]),
    "uaps_cps_fwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 5 + [C.c_float] + [_PTR] * 4 + [C.c_size_t, _PTR]),
    "uaps_cps_bwd": (C.c_int, [_PTR] * 7 + [C.c_int] * 5 + [_PTR] * 3),
    "uaps_ucc_cutmix_batch": (C.c_int, [_PTR] * 6 + [C.c_int] * 4 + [_PTR] * 3),
    "uaps_ucc_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_ucc_fwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 4 + [C.c_float] + [_PTR] * 6 + [C.c_size_t, _PTR]),
    "uaps_ucc_bwd": (C.c_int, [_PTR] * 6 + [C.c_int] * 4 + [_PTR] * 3),
    "uaps_segloss_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_segloss_fwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 4 + [_PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_segloss_bwd": (C.c_int, [_PTR] * 5 + [C.c_int] * 4 + [_PTR, _PTR]),
    "uaps_binloss_workspace_bytes": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t)]),
    "uaps_binloss_fwd": (C.c_int, [_PTR] * 3 + [C.c_int] * 3 + [_PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_binloss_bwd": (C.c_int, [_PTR] * 5 + [C.c_int] * 3 + [_PTR, _PTR]),
    "uaps_sigmoid_mse_fwd": (C.c_int, [_PTR, _PTR, C.c_long, _PTR, _PTR]),
    "uaps_sigmoid_mse_bwd": (C.c_int, [_PTR, _PTR, _PTR, C.c_long, _PTR, _PTR]),
    "uaps_sigmoid_kl_fwd": (C.c_int, [_PTR, _PTR, C.c_long, _PTR, _PTR, C.c_size_t, _PTR]),
    "uaps_sigmoid_kl_bwd": (C.c_int, [_PTR, _PTR, _PTR, C.c_long, _PTR, _PTR]),
    "uaps_bin_confusion": (C.c_int, [_PTR, _PTR] + [C.c_int] * 3 + [C.c_double, _PTR, _PTR]),
    "uaps_tta_views": (C.c_int, [_PTR]),
    "uaps_tta_fold": (C.c_int, [_PTR]),
    "uaps_instances_workspace_bytes": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t)]),
    "uaps_label_instances": (C.c_int, [_PTR]),
    "uaps_rle_count": (C.c_int, [_PTR]),
    "uaps_rle_encode": (C.c_int, [_PTR]),
    "uaps_rle_decode": (C.c_int, [_PTR]),
    "uaps_morphology": (C.c_int, [_PTR]),
    "uaps_morph_band_rows": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)]),
    "uaps_components_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_components": (C.c_int, [_PTR]),
    "uaps_hysteresis_workspace_bytes": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t)]),
    "uaps_hysteresis": (C.c_int, [_PTR]),
    "uaps_split_workspace_bytes": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t)]),
    "uaps_split_band_rows": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "uaps_split_instances": (C.c_int, [_PTR]),
    "uaps_shape_descriptors": (C.c_int, [_PTR]),
    "uaps_skeleton_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_skeleton_band_rows": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_int)]),
    "uaps_skeletonize": (C.c_int, [_PTR]),
    "uaps_skeleton_stats": (C.c_int, [_PTR]),
    "uaps_tile_origins": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]),
    "uaps_tile_cut": (C.c_int, [_PTR]),
    "uaps_tile_fold": (C.c_int, [_PTR]),
    "uaps_edt_workspace_bytes": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t)]),
    "uaps_edt_sq": (C.c_int, [_PTR]),
    "uaps_surface_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_surface_distances": (C.c_int, [_PTR]),
    "uaps_match_workspace_bytes": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t)]),
    "uaps_match_instances": (C.c_int, [_PTR]),
    "uaps_detect_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_detect_match": (C.c_int, [_PTR]),
    "uaps_curves_workspace_bytes": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_size_t)]),
    "uaps_score_curves": (C.c_int, [_PTR]),
    "uaps_plane_curves": (C.c_int, [_PTR]),
    "uaps_hull_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_hull_descriptors": (C.c_int, [_PTR]),
    "uaps_contours_workspace_bytes": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_contours_trace": (C.c_int, [_PTR]),
    "uaps_contours_write": (C.c_int, [_PTR]),
    "uaps_contours_simplify_workspace_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    "uaps_contours_simplify_mark": (C.c_int, [_PTR]),
    "uaps_contours_simplify_write": (C.c_int, [_PTR]),
    "uaps_raster_workspace_bytes": (C.c_int, [C.c_int64, C.c_int64] + [C.c_int] * 4 + [C.POINTER(C.c_size_t)]),
    "uaps_raster_plan": (C.c_int, [_PTR]),
    "uaps_raster_fill": (C.c_int, [_PTR]),
}


# The explicit-hints forms (include/uaps_hip.h, "Explicit-hints forms"): `<name>_h(const uaps_call_hints*, same arguments)`.  These are
# what the package calls; the base names stay bound for the C-ABI tests and foreign callers.
HINTED = ("uaps_conv_fwd", "uaps_conv_fwd_stats", "uaps_conv_fwd_bn", "uaps_conv_fwd_cat", "uaps_conv_bwd_data", "uaps_conv_bwd_data_cat",
          "uaps_conv_bwd_weight_partial", "uaps_conv_bwd_weight_partial_bn", "uaps_conv_bwd_weight_partial_cat",
          "uaps_bn_act_fwd_train_partials", "uaps_bn_finalize_train", "uaps_bn_act_bwd_grouped", "uaps_bn_act_bwd_grouped_bias",
          "uaps_bn_act_bwd_apply", "uaps_up_cat_fwd", "uaps_cat2", "uaps_add_relu", "uaps_pairloss_bwd", "uaps_rot90_batch", "uaps_ucc_cutmix_batch")
for _n in HINTED:
    SIGNATURES[_n + "_h"] = (SIGNATURES[_n][0], [_PTR] + list(SIGNATURES[_n][1]))
del _n
# the encoder-glue forms (include/uaps_hip.h): hinted entry points without an unhinted twin
SIGNATURES["uaps_bn_apply_pool_support"] = (C.c_int, [C.c_int, C.c_int])
SIGNATURES["uaps_bn_act_fwd_train_partials_pool_h"] = (C.c_int, list(SIGNATURES["uaps_bn_act_fwd_train_partials_h"][1]) + [_PTR, _PTR])
SIGNATURES["uaps_fanin_perturbed_bn_sums_h"] = (C.c_int, [_PTR] + list(SIGNATURES["uaps_fanin_perturbed"][1][:-1]) + [_PTR] * 5 + [C.c_float, _PTR, _PTR])
SIGNATURES["uaps_bn_act_bwd_partials_h"] = (C.c_int, [_PTR, _PTR, C.c_int] + [_PTR] * 6 + [C.c_float] + [C.c_int] * 5 + [_PTR] * 5)


class UapsHipError(RuntimeError):
    pass


def build(verbose: bool = False, jobs: int = 8) -> str:
    """Compile every HIP source under uaps_amd/csrc for gfx950 into uaps_amd/lib/libuaps_hip.so."""
    cmd = ["make", "-C", CSRC, f"-j{jobs}"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise UapsHipError("building libuaps_hip.so failed (see output above)")
    return LIB_PATH


def lib() -> C.CDLL:
    """The loaded library with typed entry points; raises UapsHipError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise UapsHipError(
                    f"{LIB_PATH} not found: the UAPS HIP kernels are not built. Run "
                    "`make -C uaps_amd/csrc` (needs hipcc; cross-compiles for gfx950 without a GPU). "
                    "uaps_amd has no CPU or PyTorch fallback for these ops.")
            l = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                try:
                    fn = getattr(l, name)
                except AttributeError as e:
                    raise UapsHipError(f"libuaps_hip.so does not export {name}; rebuild it") from e
                fn.restype, fn.argtypes = res, args
            _configure_from_environment(l)
            _lib = l
    return _lib


# planner switches of uaps_conv_set_tuning (include/uaps_hip.h: UAPS_TUNE_*) <- the environment variables the ablation and
# diagnosis scripts set; the library itself reads no environment
_TUNE_ENV = (("UAPS_DIAG_NO_SPLIT_FWD", 1, None), ("UAPS_DIAG_NO_SPLIT_WRW", 2, None), ("UAPS_DIAG_NO_SMALL", 4, None),
             ("UAPS_DIAG_NO_HP16", 8, None), ("UAPS_SWRW_COLMAJOR", 16, "0"), ("UAPS_WRW_TALL", 32, "0"), ("UAPS_FWD_TALL", 64, "0"),
             ("UAPS_DIAG_NO_ROW16", 128, None), ("UAPS_DIAG_NO_ROW_WRW", 256, None), ("UAPS_DIAG_DEEP_ROWS", 512, None),
             ("UAPS_DIAG_G1_NARROW", 1024, None), ("UAPS_DIAG_NO_G", 2048, None), ("UAPS_DIAG_G_DEEP", 4096, None))


def _configure_from_environment(l) -> None:
    mode = config.text("UAPS_CONV_MODE")
    if mode:                                    # "0" / "exact" / "f32";  "1" / "bf16" / "split";  "2" / "h16"
        m = 0 if mode[0] in "0ef" else (1 if mode[0] in "1bs" else 2)
        if l.uaps_conv_set_mode(m) != 0:
            raise UapsHipError(f"UAPS_CONV_MODE={mode}: uaps_conv_set_mode failed")
    flags = 0
    for name, bit, on_value in _TUNE_ENV:
        v = config.text(name)
        if v is not None and (on_value is None or v == on_value):
            flags |= bit
    l.uaps_conv_set_tuning(flags)


class quiet_gc:
    """Around a hipGraph capture: collect garbage first and keep the cyclic collector off while the stream captures.  The step's
    capture runs thousands of lines of Python; a collection in the middle of it finalises whatever dead cycles the process holds --
    other trainers' CUDAGraph objects (hipGraphExecDestroy), tensors of other private pools -- i.e. runtime calls from inside a
    global-mode capture.  torch.cuda.graph() used to collect before capturing and no longer does (torch.compiler.config.
    force_cudagraph_gc, off by default); seen as an intermittent segmentation fault in capture_end in a test process that had
    built and dropped a dozen captured trainers."""

    def __enter__(self):
        import gc
        gc.collect()
        self.was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self.was:
            gc.enable()
        return False


class WrwReduceItem(C.Structure):
    """uaps_wrw_reduce_item (include/uaps_hip.h)."""
    _fields_ = [("workspace", C.c_void_p), ("dw", C.c_void_p), ("dbias", C.c_void_p), ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("H", C.c_int), ("W", C.c_int), ("ks", C.c_int), ("cfg", C.c_int)]


class CallHints(C.Structure):
    """uaps_call_hints (include/uaps_hip.h): the optional operands of ONE call, handed to the *_h entry points as their first argument."""
    _fields_ = [("struct_size", C.c_uint), ("bound", C.c_void_p * 3), ("mul", C.c_float * 3), ("out_amax", C.c_void_p),
                ("stats_mean", C.c_void_p), ("stats_bias", C.c_void_p), ("residual", C.c_void_p),
                ("dyt_y", C.c_void_p), ("dyt_coef", C.c_void_p), ("dyt_out", C.c_void_p), ("dyt_slope", C.c_float), ("dyt_groups", C.c_int),
                ("bsum_y", C.c_void_p), ("bsum_mean", C.c_void_p), ("bsum_invstd", C.c_void_p), ("bsum_gamma", C.c_void_p),
                ("bsum_beta", C.c_void_p), ("bsum_partials", C.c_void_p), ("bsum_max", C.c_void_p), ("bsum_slope", C.c_float),
                ("bsum_groups", C.c_int)]


class ConvCall(C.Structure):
    """uaps_conv_call (include/uaps_hip.h): the explicit, size-versioned form of the convolution entry points (uaps_conv_ex)."""
    _fields_ = [("struct_size", C.c_uint), ("op", C.c_int), ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("H", C.c_int),
                ("W", C.c_int), ("ks", C.c_int), ("cfg", C.c_int), ("x", C.c_void_p), ("C1", C.c_int), ("x2", C.c_void_p),
                ("w_packed", C.c_void_p), ("bias", C.c_void_p), ("y", C.c_void_p), ("y2", C.c_void_p), ("y_grad", C.c_void_p),
                ("stats", C.c_void_p), ("xf", C.c_void_p), ("xf_slope", C.c_float), ("xf_groups", C.c_int), ("want_bias", C.c_int),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p), ("hints", CallHints)]


AUG_MAX_OPS = 8                         # UAPS_AUG_MAX_OPS
AUG_END, AUG_BC, AUG_NOISE, AUG_BLUR, AUG_BRIGHT, AUG_CONTRAST, AUG_SATURATE, AUG_HUE, AUG_PIXDROP, AUG_GRID = range(10)   # UAPS_AUG_*


class ViewRow(C.Structure):
    """uaps_view_row (include/uaps_hip.h): the geometry row and the program of one (view, image)."""
    _fields_ = [("hflip", C.c_int32), ("vflip", C.c_int32), ("rot_k", C.c_int32), ("grid_on", C.c_int32),
                ("op", C.c_int32 * AUG_MAX_OPS), ("a", C.c_float * AUG_MAX_OPS), ("b", C.c_float * AUG_MAX_OPS)]


class AugmentViewsCall(C.Structure):
    """uaps_augment_views_call (include/uaps_hip.h): every operand of uaps_augment_views, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("V", C.c_int32), ("B", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("Cs", C.c_int32),
                ("Ho", C.c_int32), ("Wo", C.c_int32), ("images", C.c_void_p), ("masks", C.c_void_p), ("rows_host", C.c_void_p),
                ("rows", C.c_void_p), ("grid_ys", C.c_void_p), ("grid_xs", C.c_void_p), ("noise", C.c_void_p), ("drop_u", C.c_void_p),
                ("seed", C.c_uint64), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("out", C.c_void_p), ("out_mask", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


TTA_MAX_SCALES = 8                      # UAPS_TTA_MAX_SCALES


class TTAViewsCall(C.Structure):
    """uaps_tta_views_call (include/uaps_hip.h): every operand of uaps_tta_views, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("Cin", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("h", C.c_int32),
                ("w", C.c_int32), ("flip", C.c_int32), ("x", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


class TTAFoldCall(C.Structure):
    """uaps_tta_fold_call (include/uaps_hip.h): every operand of uaps_tta_fold, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("S", C.c_int32), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("flip", C.c_int32), ("logits", C.c_void_p * TTA_MAX_SCALES), ("h", C.c_int32 * TTA_MAX_SCALES),
                ("w", C.c_int32 * TTA_MAX_SCALES), ("probs_sum", C.c_void_p), ("mask", C.c_void_p), ("conf", C.c_void_p),
                ("stream", C.c_void_p)]


class InstancesCall(C.Structure):
    """uaps_instances_call (include/uaps_hip.h): every operand of uaps_label_instances, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("connectivity", C.c_int32),
                ("has_background", C.c_int32), ("background", C.c_int64), ("min_area", C.c_int32), ("max_instances", C.c_int32),
                ("mask", C.c_void_p), ("map0", C.c_void_p), ("map1", C.c_void_p), ("labels", C.c_void_p), ("count", C.c_void_p),
                ("table", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


RLE_MAX_CLASSES = 8                     # UAPS_RLE_MAX_CLASSES


class RleCall(C.Structure):
    """uaps_rle_call (include/uaps_hip.h): the operands of uaps_rle_count / _encode / _decode, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_classes", C.c_int32),
                ("classes", C.c_int64 * RLE_MAX_CLASSES), ("mask", C.c_void_p), ("col_offsets", C.c_void_p), ("pairs", C.c_void_p),
                ("offsets", C.c_void_p), ("n_runs", C.c_int64), ("out", C.c_void_p), ("out_uint8", C.c_int32), ("stream", C.c_void_p)]


MORPH_MAX_STEPS, MORPH_MAX_CLASSES = 8, 8   # UAPS_MORPH_MAX_STEPS, UAPS_MORPH_MAX_CLASSES
MORPH_OPS = {"erode": 0, "dilate": 1, "open": 2, "close": 3, "boundary": 4}     # UAPS_MORPH_ERODE ..
MORPH_FOOTPRINTS = {"square": 0, "cross": 1, "disk": 2}                         # UAPS_MORPH_SQUARE ..


class MorphCall(C.Structure):
    """uaps_morph_call (include/uaps_hip.h): every operand of uaps_morphology, size-versioned."""
    _fields_ = [("struct_size", C.c_size_t), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_steps", C.c_int32),
                ("op", C.c_int32 * MORPH_MAX_STEPS), ("footprint", C.c_int32 * MORPH_MAX_STEPS), ("radius", C.c_int32 * MORPH_MAX_STEPS),
                ("n_classes", C.c_int32), ("classes", C.c_int32 * MORPH_MAX_CLASSES), ("background", C.c_int32),
                ("band_rows", C.c_int32), ("mask", C.c_void_p), ("out", C.c_void_p), ("stream", C.c_void_p)]


COMP_MAX_STEPS, COMP_MAX_CLASSES, COMP_ALL = 8, 8, 2 ** 31 - 1       # UAPS_COMP_MAX_STEPS, UAPS_COMP_MAX_CLASSES, UAPS_COMP_ALL
COMP_KINDS = {"area_open": 0, "clear_border": 1, "fill_holes": 2}      # UAPS_COMP_AREA_OPEN ..


class ComponentsCall(C.Structure):
    """uaps_components_call (include/uaps_hip.h): every operand of uaps_components, size-versioned."""
    _fields_ = [("struct_size", C.c_size_t), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_steps", C.c_int32),
                ("kind", C.c_int32 * COMP_MAX_STEPS), ("n", C.c_int32 * COMP_MAX_STEPS), ("n_classes", C.c_int32),
                ("classes", C.c_int32 * COMP_MAX_CLASSES), ("background", C.c_int32), ("connectivity", C.c_int32),
                ("mask", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


HYST_MAX_CLASSES = 8                    # UAPS_HYST_MAX_CLASSES


class HysteresisCall(C.Structure):
    """uaps_hysteresis_call (include/uaps_hip.h): every operand of uaps_hysteresis, size-versioned."""
    _fields_ = [("struct_size", C.c_size_t), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("from_logits", C.c_int32), ("n_classes", C.c_int32), ("classes", C.c_int32 * HYST_MAX_CLASSES),
                ("low", C.c_float * HYST_MAX_CLASSES), ("high", C.c_float * HYST_MAX_CLASSES), ("background", C.c_int32),
                ("connectivity", C.c_int32), ("min_area", C.c_int32), ("scores", C.c_void_p), ("mask", C.c_void_p),
                ("markers", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


SPLIT_MAX_EXTENT, SPLIT_MAX_ITERS, SPLIT_MAX_SUB_ITERS = 4096, 65536, 16     # UAPS_SPLIT_*


class SplitCall(C.Structure):
    """uaps_split_call (include/uaps_hip.h): every operand of uaps_split_instances, size-versioned."""
    _fields_ = [("struct_size", C.c_size_t), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("connectivity", C.c_int32),
                ("d2", C.c_int32), ("min_marker_area", C.c_int32), ("max_iters", C.c_int32), ("sub_iters", C.c_int32),
                ("band_rows", C.c_int32), ("tile_cols", C.c_int32), ("min_area", C.c_int32), ("max_instances", C.c_int32),
                ("source_rows", C.c_int32), ("source_labels", C.c_void_p), ("source_table", C.c_void_p), ("distance", C.c_void_p),
                ("markers", C.c_void_p), ("map0", C.c_void_p), ("map1", C.c_void_p), ("labels", C.c_void_p), ("count", C.c_void_p),
                ("table", C.c_void_p), ("parent", C.c_void_p), ("pieces", C.c_void_p), ("converged", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


SHAPE_COLUMNS, SHAPE_MAX_EXTENT, SHAPE_LDS_ROWS = 11, 16384, 256     # UAPS_SHAPE_COLUMNS, UAPS_SHAPE_MAX_EXTENT, UAPS_SHAPE_LDS_ROWS


class ShapeCall(C.Structure):
    """uaps_shape_call (include/uaps_hip.h): every operand of uaps_shape_descriptors, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("max_instances", C.c_int32),
                ("labels", C.c_void_p), ("plane", C.c_void_p), ("table", C.c_void_p), ("stream", C.c_void_p)]


SKEL_MAX_CLASSES, SKEL_MAX_ITERS, SKEL_MAX_SUB_ITERS, SKEL_MAX_EXTENT, SKEL_COLUMNS = 8, 2048, 64, 4096, 7       # UAPS_SKEL_*


class SkeletonCall(C.Structure):
    """uaps_skeleton_call (include/uaps_hip.h): every operand of uaps_skeletonize, size-versioned."""
    _fields_ = [("struct_size", C.c_size_t), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_classes", C.c_int32),
                ("classes", C.c_int32 * SKEL_MAX_CLASSES), ("background", C.c_int32), ("max_iters", C.c_int32),
                ("sub_iters", C.c_int32), ("band_rows", C.c_int32), ("mask", C.c_void_p), ("out", C.c_void_p),
                ("converged", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class SkeletonStatsCall(C.Structure):
    """uaps_skeleton_stats_call (include/uaps_hip.h): every operand of uaps_skeleton_stats, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("max_instances", C.c_int32),
                ("n_classes", C.c_int32), ("classes", C.c_int32 * SKEL_MAX_CLASSES), ("labels", C.c_void_p), ("skel", C.c_void_p),
                ("plane", C.c_void_p), ("table", C.c_void_p), ("stream", C.c_void_p)]


HULL_COLUMNS, HULL_MAX_EXTENT = 17, 4096       # UAPS_HULL_COLUMNS, UAPS_HULL_MAX_EXTENT


class HullCall(C.Structure):
    """uaps_hull_call (include/uaps_hip.h): every operand of uaps_hull_descriptors, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("max_instances", C.c_int32),
                ("labels", C.c_void_p), ("table", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


CONTOUR_COLUMNS, CONTOUR_RING_COLUMNS, CONTOUR_MAX_EXTENT = 4, 7, 4096     # UAPS_CONTOUR_COLUMNS, _RING_COLUMNS, _MAX_EXTENT


class ContourCall(C.Structure):
    """uaps_contour_call (include/uaps_hip.h): every operand of uaps_contours_trace and uaps_contours_write, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("max_instances", C.c_int32),
                ("connectivity", C.c_int32), ("labels", C.c_void_p), ("summary", C.c_void_p), ("totals", C.c_void_p),
                ("n_rings", C.c_int64), ("n_points", C.c_int64), ("ring_capacity", C.c_int64), ("point_capacity", C.c_int64),
                ("points", C.c_void_p), ("ring_offsets", C.c_void_p), ("rings", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


SIMPLIFY_WAVE_MAX, SIMPLIFY_LDS_MAX, SIMPLIFY_MAX_E16, SIMPLIFY_OFF = 64, 2048, 1024, -1     # UAPS_SIMPLIFY_*


class SimplifyCall(C.Structure):
    """uaps_simplify_call (include/uaps_hip.h): every operand of uaps_contours_simplify_mark and _write, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("max_instances", C.c_int32), ("e16", C.c_int32),
                ("wave_max", C.c_int32), ("lds_max", C.c_int32), ("n_points", C.c_int64), ("n_rings", C.c_int64),
                ("points", C.c_void_p), ("ring_offsets", C.c_void_p), ("rings", C.c_void_p), ("summary_in", C.c_void_p),
                ("summary_out", C.c_void_p), ("totals", C.c_void_p), ("n_points_out", C.c_int64), ("ring_capacity", C.c_int64),
                ("point_capacity", C.c_int64), ("points_out", C.c_void_p), ("ring_offsets_out", C.c_void_p), ("rings_out", C.c_void_p),
                ("ring_stats", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


RASTER_COLUMNS, RASTER_MAX_EXTENT, RASTER_MAX_FRAC_BITS, RASTER_WAVE_ROWS, RASTER_ALL_WAVE = 2, 4096, 4, 64, -1     # UAPS_RASTER_*


class RasterCall(C.Structure):
    """uaps_raster_call (include/uaps_hip.h): every operand of uaps_raster_plan and uaps_raster_fill, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("max_instances", C.c_int32),
                ("frac_bits", C.c_int32), ("ring_stride", C.c_int32), ("edge_wave_rows", C.c_int32), ("n_points", C.c_int64),
                ("n_rings", C.c_int64), ("points", C.c_void_p), ("ring_offsets", C.c_void_p), ("rings", C.c_void_p),
                ("totals", C.c_void_p), ("n_words", C.c_int64), ("planes", C.c_void_p), ("reference", C.c_void_p),
                ("classes", C.c_void_p), ("background", C.c_int64), ("labels", C.c_void_p), ("mask", C.c_void_p),
                ("stats", C.c_void_p), ("overlap", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


TILE_MAX_CHUNKS, TILE_MAX_MAPS = 32, 2  # UAPS_TILE_MAX_CHUNKS, UAPS_TILE_MAX_MAPS


class TileCutCall(C.Structure):
    """uaps_tile_cut_call (include/uaps_hip.h): every operand of uaps_tile_cut, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("Cin", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("th", C.c_int32),
                ("tw", C.c_int32), ("oy", C.c_int32), ("ox", C.c_int32), ("g0", C.c_int32), ("g1", C.c_int32), ("x", C.c_void_p),
                ("out", C.c_void_p), ("stream", C.c_void_p)]


class TileFoldCall(C.Structure):
    """uaps_tile_fold_call (include/uaps_hip.h): every operand of uaps_tile_fold, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("th", C.c_int32),
                ("tw", C.c_int32), ("oy", C.c_int32), ("ox", C.c_int32), ("n_chunks", C.c_int32), ("tiles_per_chunk", C.c_int32),
                ("n_maps", C.c_int32), ("logits", C.c_void_p * TILE_MAX_CHUNKS), ("maps", (C.c_void_p * TILE_MAX_CHUNKS) * TILE_MAX_MAPS),
                ("wy", C.c_void_p), ("wx", C.c_void_p), ("probs", C.c_void_p), ("mask", C.c_void_p), ("conf", C.c_void_p),
                ("map_out", C.c_void_p * TILE_MAX_MAPS), ("stream", C.c_void_p)]


class EdtCall(C.Structure):
    """uaps_edt_call (include/uaps_hip.h): every operand of uaps_edt_sq, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("mask_dtype", C.c_int32),
                ("mask", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class SurfaceCall(C.Structure):
    """uaps_surface_call (include/uaps_hip.h): every operand of uaps_surface_distances, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("pred_dtype", C.c_int32), ("target_dtype", C.c_int32), ("pred", C.c_void_p), ("pred_scores", C.c_void_p),
                ("target", C.c_void_p), ("percentile_frac", C.c_double), ("has_tolerance", C.c_int32), ("tol_d2", C.c_int64),
                ("table", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


MATCH_MAX_CLASSES, MATCH_COLUMNS = 64, 4  # UAPS_MATCH_MAX_CLASSES, UAPS_MATCH_COLUMNS


class MatchCall(C.Structure):
    """uaps_match_call (include/uaps_hip.h): every operand of uaps_match_instances, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("num_classes", C.c_int32),
                ("class_agnostic", C.c_int32), ("iou_threshold", C.c_double), ("pred_labels", C.c_void_p), ("target_labels", C.c_void_p),
                ("pred_count", C.c_void_p), ("target_count", C.c_void_p), ("pred_table", C.c_void_p), ("target_table", C.c_void_p),
                ("max_pred", C.c_int32), ("max_gt", C.c_int32), ("pred_out", C.c_void_p), ("target_out", C.c_void_p),
                ("counts", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


DETECT_MAX_THRESHOLDS, DETECT_MAX_CANDIDATES, DETECT_MAX_ROWS = 32, 10, 4096     # UAPS_DETECT_MAX_*


class DetectCall(C.Structure):
    """uaps_detect_call (include/uaps_hip.h): every operand of uaps_detect_match, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("num_classes", C.c_int32),
                ("class_agnostic", C.c_int32), ("T", C.c_int32), ("max_dets", C.c_int32), ("t1000", C.c_int32 * DETECT_MAX_THRESHOLDS),
                ("pred_labels", C.c_void_p), ("target_labels", C.c_void_p), ("pred_count", C.c_void_p), ("target_count", C.c_void_p),
                ("pred_table", C.c_void_p), ("target_table", C.c_void_p), ("max_pred", C.c_int32), ("max_gt", C.c_int32),
                ("scores", C.c_void_p), ("score", C.c_void_p), ("rank", C.c_void_p), ("pred_match", C.c_void_p),
                ("pred_inter", C.c_void_p), ("target_match", C.c_void_p), ("counts", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


CURVES_MAX_BINS = 4096                  # UAPS_CURVES_MAX_BINS


class CurvesCall(C.Structure):
    """uaps_curves_call (include/uaps_hip.h): every operand of uaps_score_curves, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("bins", C.c_int32),
                ("from_logits", C.c_int32), ("top_row", C.c_int32), ("n_classes", C.c_int32), ("classes", C.c_int32 * 8),
                ("target_dtype", C.c_int32), ("lo", C.c_float), ("hi", C.c_float), ("scores", C.c_void_p), ("target", C.c_void_p),
                ("region_labels", C.c_void_p), ("region_count", C.c_void_p), ("region_table", C.c_void_p), ("max_regions", C.c_int32),
                ("hist", C.c_void_p), ("qsum", C.c_void_p), ("nan", C.c_void_p), ("pro_sum", C.c_void_p), ("n_regions", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


class PlaneCurvesCall(C.Structure):
    """uaps_plane_curves_call (include/uaps_hip.h): every operand of uaps_plane_curves, size-versioned."""
    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("bins", C.c_int32),
                ("from_logits", C.c_int32), ("pred_dtype", C.c_int32), ("target_dtype", C.c_int32), ("lo", C.c_float), ("hi", C.c_float),
                ("score", C.c_void_p), ("pred", C.c_void_p), ("target", C.c_void_p), ("hist", C.c_void_p), ("qsum", C.c_void_p),
                ("nan", C.c_void_p), ("stream", C.c_void_p)]


SEG_NTERMS, SEG_MAX_CLASSES = 6, 8      # UAPS_SEG_NTERMS, UAPS_MAX_CLASSES


def seg_nscalars(Cc: int) -> int:
    """UAPS_SEG_S_NSCALARS(C) (include/uaps_hip.h)."""
    return 16 + 7 * Cc


class SegLossParams(C.Structure):
    """uaps_segloss_params (include/uaps_hip.h): passed by value into the kernels of uaps_segloss_fwd / _bwd."""
    _fields_ = [("struct_size", C.c_uint32), ("terms", C.c_uint32), ("coef", C.c_float * SEG_NTERMS),
                ("class_weight", C.c_float * SEG_MAX_CLASSES), ("focal_alpha", C.c_float * SEG_MAX_CLASSES), ("focal_gamma", C.c_float),
                ("focal_mean", C.c_int), ("dice_sq_weight", C.c_float * SEG_MAX_CLASSES), ("tversky_alpha", C.c_float),
                ("tversky_beta", C.c_float), ("eps", C.c_float), ("smooth", C.c_float), ("ignore_index", C.c_int64)]


BIN_NTERMS, BIN_NSCALARS = 7, 24       # UAPS_BIN_NTERMS, UAPS_BIN_S_NSCALARS


class BinLossParams(C.Structure):
    """uaps_binloss_params (include/uaps_hip.h): passed by value into the kernels of uaps_binloss_fwd / _bwd."""
    _fields_ = [("struct_size", C.c_uint32), ("terms", C.c_uint32), ("coef", C.c_float * BIN_NTERMS), ("target_float", C.c_uint32),
                ("has_pos_weight", C.c_uint32), ("pos_weight", C.c_float), ("focal_alpha", C.c_float), ("focal_gamma", C.c_float),
                ("focal_mean", C.c_int), ("beta", C.c_float), ("tversky_alpha", C.c_float), ("tversky_beta", C.c_float),
                ("eps", C.c_float)]


def mk_hints(bounds=(), out_amax=None, stats=None, residual=None, dyt=None, bsum=None):
    """The uaps_call_hints argument of a *_h entry point (a ctypes byref; pass None for "no hints").
    bounds: up to three (bound tensor, host factor) pairs or None; out_amax: a zeroed bound tensor; stats: (running_mean or
    None, conv bias or None) = the per-channel shift BatchNorm partial sums are formed about / were formed about; residual: the
    tensor a BatchNorm apply pass adds before its ReLU (residual joins).
    The record is an ARGUMENT: the library copies it inside the call it is passed to and keeps nothing.  The buffer behind the returned
    reference is this Python thread's and is rewritten by the next mk_hints of the thread, so build it in the call expression."""
    h = getattr(_tls, "hints", None)
    if h is None:
        h = _tls.hints = CallHints()
        h.struct_size = C.sizeof(CallHints)
    for i in range(3):
        h.bound[i] = None
    h.out_amax = h.stats_mean = h.stats_bias = None
    h.residual = residual.data_ptr() if residual is not None else None
    if dyt is not None:                       # (y, coef, out, slope, groups): uaps_call_hints::dyt_* (uaps_bn_act_bwd_prepare)
        h.dyt_y, h.dyt_coef, h.dyt_out, h.dyt_slope, h.dyt_groups = dyt[0].data_ptr(), dyt[1].data_ptr(), dyt[2].data_ptr(), float(dyt[3]), int(dyt[4])
    else:
        h.dyt_y = h.dyt_coef = h.dyt_out = None
        h.dyt_slope, h.dyt_groups = 0.0, 0
    if bsum is not None:                      # (y, mean, invstd, gamma, beta, partials, maxes, slope, groups): uaps_call_hints::bsum_*
        (h.bsum_y, h.bsum_mean, h.bsum_invstd, h.bsum_gamma, h.bsum_beta, h.bsum_partials, h.bsum_max) = [t.data_ptr() for t in bsum[:7]]
        h.bsum_slope, h.bsum_groups = float(bsum[7]), int(bsum[8])
    else:
        h.bsum_y = h.bsum_mean = h.bsum_invstd = h.bsum_gamma = h.bsum_beta = h.bsum_partials = h.bsum_max = None
        h.bsum_slope, h.bsum_groups = 0.0, 0
    if stats is not None:
        if stats[0] is not None:
            h.stats_mean = stats[0].data_ptr()
        if stats[1] is not None:
            h.stats_bias = stats[1].data_ptr()
    for i, b in enumerate(bounds):
        if b is not None:
            h.bound[i], h.mul[i] = b[0].data_ptr(), float(b[1])
    if out_amax is not None:
        h.out_amax = out_amax.data_ptr()
    return C.byref(h)


class LaunchTimer:
    """Times the MAIN kernel launched by the entry point(s) called inside the `with` block: the two events are attached to
    that kernel's dispatch (uaps_next_launch_events), so `elapsed_ms()` after a synchronize is the kernel's execution time
    as rocprofv3's kernel trace reports it.  When no main launch consumed them (an entry point without one), they bracket
    the block on the stream instead (event-to-event: includes the launch gaps)."""

    def __enter__(self):
        import torch
        self.start, self.stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.start.record()                 # creates the hipEvent_t; also the start mark of the fall-back
        self.stop.record()
        lib().uaps_next_launch_events(self.start.cuda_event, self.stop.cuda_event)
        return self

    def __exit__(self, *a):
        self.dispatch = bool(lib().uaps_next_launch_events(None, None))
        if not self.dispatch:
            self.stop.record()
        return False

    def elapsed_ms(self) -> float:
        return self.start.elapsed_time(self.stop)


_error_words = {}      # device index -> int32[1] tensor, never freed (the library holds its raw pointer)


def error_word(device):
    """The sticky error word of `device` (include/uaps_hip.h, uaps_set_error_word): allocated once per device, bound for good and
    never freed, so that the raw pointer the library keeps cannot dangle whatever happens to trainers and models.  Shared by
    everything that runs on the device; UAPSTrainer.check_errors reads and clears it."""
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    w = _error_words.get(idx)
    if w is None:
        w = _error_words[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    with torch.cuda.device(idx):           # (re)bound on every call: a caller of the C ABI may have pointed the library elsewhere
        check(lib().uaps_set_error_word(w.data_ptr()), "uaps_set_error_word")
    return w


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().uaps_error_string(rc).decode()
        raise UapsHipError(f"{what} failed: {msg} (code {rc})")


def ptr_array(tensors):
    """Host array of device pointers (const float* const*)."""
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def current_stream(device=None) -> int:
    """Raw hipStream_t of torch's current stream on `device` (fast path: no Stream object is built)."""
    import torch
    if device is None:
        idx = torch.cuda.current_device()
    else:
        idx = device.index if isinstance(device, torch.device) else int(device)
        if idx is None:
            idx = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


class Workspace:
    """Scratch for a module's kernels: one uint8 buffer per (device index, raw stream), grown on demand (to at least `min_bytes`),
    never shrunk, never freed.  Every module keeps an instance of its own -- captured graphs hold these pointers, and kernels of
    different modules are in flight on one stream at once."""
    __slots__ = ("min_bytes", "bufs", "torch")

    def __init__(self, min_bytes: int = 0):
        import torch
        self.min_bytes, self.bufs, self.torch = int(min_bytes), {}, torch

    def get(self, device, nbytes: int):
        torch = self.torch
        idx = device.index
        if idx is None:
            idx = torch.cuda.current_device()
        key = (idx, torch._C._cuda_getCurrentRawStream(idx))
        w = self.bufs.get(key)
        if w is None or w.numel() < nbytes:
            w = self.bufs[key] = torch.empty(max(nbytes, self.min_bytes), dtype=torch.uint8, device=device)
        return w


class device_guard:
    """`with device_guard(dev):` = torch.cuda.device(dev), skipped when dev already is the current device (the usual
    case: one process per GPU), which saves a few microseconds on each of the ~700 launches of a step."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        import torch
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self.ctx = None if idx == torch.cuda.current_device() else torch.cuda.device(idx)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()
        return self

    def __exit__(self, *a):
        if self.ctx is not None:
            return self.ctx.__exit__(*a)
        return False


def workspace_bytes(name: str, *dims) -> int:
    """What the size query `name` (a uaps_*_workspace_bytes entry point) answers for `dims`."""
    need = C.c_size_t()
    check(getattr(lib(), name)(*dims, C.byref(need)), name)
    return need.value


def _fill(array, values) -> None:
    for i, v in enumerate(values):
        if isinstance(v, (list, tuple)):
            _fill(array[i], v)
        else:
            array[i] = v


def call(name: str, struct, device, workspace: Workspace = None, nbytes: int = 0, **fields) -> None:
    """One call of the entry point `name`, which takes a size-versioned struct (the *_call records of include/uaps_hip.h): builds a
    `struct`, sets struct_size, the given fields (a list or tuple fills an array field from its start), with `workspace` (the calling
    module's own) its buffer of at least `nbytes` on the current stream, and the stream; runs under device_guard and checks the code."""
    c = struct()
    c.struct_size = C.sizeof(struct)
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            _fill(getattr(c, k), v)
        else:
            setattr(c, k, v)
    with device_guard(device):
        if workspace is not None:
            ws = workspace.get(device, nbytes)
            c.workspace, c.workspace_bytes = ws.data_ptr(), ws.numel()
        c.stream = current_stream(device)
        check(getattr(lib(), name)(C.byref(c)), name)


def require_device(t, what: str):
    """The kernels only exist for the GPU: refuse CPU tensors loudly instead of computing elsewhere."""
    if not t.is_cuda:
        raise UapsHipError(f"{what}: tensor is on {t.device}; uaps_amd ops run only on a ROCm device "
                           "(hand-written HIP kernels, no CPU fallback)")
