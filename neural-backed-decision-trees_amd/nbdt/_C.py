"""ctypes binding of libnbdt_hip.so (include/nbdt_hip.h).

There is NO CPU fallback: if the shared library is missing, or a call is made without a HIP
device, the product path raises.  (The CPU oracle under ``oracle/`` is test infrastructure and
is never imported from here.)
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np
import torch

_LIBPATH = os.environ.get("NBDT_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                         "libnbdt_hip.so")   # env: kernel A/B builds only
_lib = None

NBDT_F32, NBDT_BF16, NBDT_F16 = 0, 1, 2
NBDT_U8 = 3                     # nbdt_augment_batch's src_dtype for a uint8 dataset
NBDT_SD_MAX_UNITS = 64          # nbdt_stochastic_depth_draw: the longest prob / scale table
NBDT_AUGMENT_MAX_PAD = 32
NBDT_RESIZED_CROP_RATIOS = 4096     # entries of nbdt_resized_crop_batch's aspect-ratio table
NBDT_RESIZED_CROP_ATTEMPTS = 10
NBDT_POLICY_NONE, NBDT_POLICY_TA_WIDE = 0, 1
NBDT_POLICY_OPS = 14               # nbdt_policy_batch: TrivialAugmentWide's operations ...
NBDT_POLICY_BINS = 31               # ... and magnitude bins
NBDT_CHAIN_OPS = 15                 # nbdt_policy_chain_batch: the 14 and Invert
NBDT_CHAIN_MAX_OPS = 4              # slots of a chain
NBDT_CHAIN_MAX_BINS = 31
NBDT_CHAIN_MAX_SUBPOLICIES = 1024
NBDT_CHAIN_RAND, NBDT_CHAIN_SUBPOLICY = 0, 1
NBDT_CHAIN_TA_WIDE = 2              # nbdt_resized_crop_policy_batch only: one slot, nbdt_policy_batch's draw
NBDT_RESIZED_CROP_POLICY_MAX_SIDE = 512
NBDT_LINKAGE = {"ward": 0, "complete": 1, "single": 2, "average": 3}        # nbdt_linkage's method ...
NBDT_METRIC = {"euclidean": 0, "l2": 0, "manhattan": 1, "l1": 1, "cityblock": 1, "cosine": 2}     # ... and metric
_ZTYPE = {torch.float32: NBDT_F32, torch.bfloat16: NBDT_BF16, torch.float16: NBDT_F16}


class NBDTHipError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [
        ("B", c_int32), ("gh", c_int32), ("gw", c_int32),
        ("cin", c_int32), ("cout", c_int32),
        ("ntaps", c_int32),
        ("tap_off", c_int32 * 9), ("w_tap", c_int32 * 9), ("w_ntaps", c_int32),
        ("in_bs", c_int32), ("in_hs", c_int32), ("in_ws", c_int32), ("in_base", c_int32),
        ("out_bs", c_int32), ("out_hs", c_int32), ("out_ws", c_int32), ("out_base", c_int32),
        ("accumulate", c_int32),
        ("wide_tile", c_int32),
        ("ksplit", c_int32),
        ("w_tiled", ctypes.c_uint64),
    ]


class WgradDesc(ctypes.Structure):
    _fields_ = [
        ("B", c_int32), ("gh", c_int32), ("gw", c_int32),
        ("cin", c_int32), ("cout", c_int32),
        ("ntaps", c_int32),
        ("tap_off", c_int32 * 9), ("w_tap", c_int32 * 9), ("w_ntaps", c_int32),
        ("x_bs", c_int32), ("x_hs", c_int32), ("x_ws", c_int32), ("x_base", c_int32),
        ("g_bs", c_int32), ("g_hs", c_int32), ("g_ws", c_int32), ("g_base", c_int32),
        ("variant", c_int32),
        ("cu_budget", c_int32),
    ]


class TreeStats(ctypes.Structure):
    """nbdt_tree_stats: device pointers of the int64 counters nbdt_tree_stats_accumulate adds to (NULL = not wanted)."""
    FIELDS = ("totals", "confusion_net", "confusion_hard", "confusion_soft", "node_counts", "node_entropy",
              "first_error_depth")
    _fields_ = [(name, c_void_p) for name in FIELDS]


class ConvSegSlice(ctypes.Structure):
    _fields_ = [("tensor", c_int32), ("ch0", c_int32), ("ntaps", c_int32), ("tap", c_int32 * 9),
                ("w_matrix", c_int32), ("w_off", c_int32 * 9)]


class ConvSegClass(ctypes.Structure):
    _fields_ = [("nslices", c_int32), ("slices", POINTER(ConvSegSlice)),
                ("out_bs", c_int32), ("out_hs", c_int32), ("out_ws", c_int32), ("out_base", c_int32)]


class ConvSegDesc(ctypes.Structure):
    _fields_ = [("B", c_int32), ("gh", c_int32), ("gw", c_int32), ("cout", c_int32),
                ("ntensors", c_int32), ("pix_stride", c_int32 * 4),
                ("nmatrices", c_int32), ("w_row_stride", c_int32 * 4),
                ("nclasses", c_int32), ("cls", ConvSegClass * 4),
                ("tile", c_int32), ("nbuf", c_int32)]


_P = c_void_p
_I32P = POINTER(c_int32)

# name -> (restype, argtypes): every symbol include/nbdt_hip.h declares
SIGNATURES = {
    "nbdt_last_error": (c_char_p, []),
    "nbdt_version": (c_int, []),
    "nbdt_device_count": (c_int, []),
    "nbdt_set_deterministic": (c_int, [c_int32]),
    "nbdt_get_deterministic": (c_int, []),
    "nbdt_set_wgrad_store_epilogue": (c_int, [c_int32]),
    "nbdt_get_wgrad_store_epilogue": (c_int, []),
    "nbdt_set_reserved_cus": (c_int, [c_int32]),
    "nbdt_probe_mfma_stream": (c_int, [c_int32, c_int32, _P, _P]),
    "nbdt_probe_lds_mfma": (c_int, [c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_get_reserved_cus": (c_int, []),
    "nbdt_set_stream_nt_min_bytes": (c_int, [c_int64]),
    "nbdt_get_stream_nt_min_bytes": (c_int64, []),
    "nbdt_debug_last_stream_nt": (c_int, []),
    "nbdt_tree_create": (c_int, [c_int, c_int, c_int, c_int, _I32P, _I32P, _I32P, _I32P, _I32P, _I32P,
                                 POINTER(c_void_p)]),
    "nbdt_tree_destroy": (c_int, [c_void_p]),
    "nbdt_tree_max_depth": (c_int, [c_void_p]),
    "nbdt_debug_last_igemm": (c_char_p, []),
    "nbdt_debug_last_igemm_full": (c_char_p, []),
    "nbdt_debug_last_wgrad": (c_char_p, []),
    "nbdt_debug_last_rules_path": (c_char_p, []),
    "nbdt_set_rules_path": (c_int, [c_int]),
    "nbdt_get_rules_path": (c_int, []),
    "nbdt_conv_wgrad_blocks": (c_int, [_P]),
    "nbdt_conv_plan": (c_int, [_P, _P, _P]),
    "nbdt_soft_forward": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P]),
    "nbdt_soft_backward": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P, _P]),
    "nbdt_soft_tree_loss": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, c_float, c_float, c_float,
                                    _P, _P, _P, _P]),
    "nbdt_head_soft_tree_loss": (c_int, [c_void_p, _P, _P, _P, c_int64, c_int32, _P, c_float, c_float, c_float,
                                         _P, _P, _P, _P, _P, _P, _P]),
    "nbdt_hard_tree_loss": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, c_float, c_float, c_float,
                                    _P, _P, _P, _P]),
    "nbdt_soft_tree_loss_ex": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P, c_int64, c_float, c_float, c_float,
                                       c_float, _P, _P, _P, _P]),
    "nbdt_hard_tree_loss_ex": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, c_float, c_float, c_float, c_float,
                                       _P, _P, _P, _P]),
    "nbdt_mix_batch": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_float, c_float, c_int32, c_int32, c_int32, c_int32,
                               c_float, c_float, _P, _P, c_int32, _P]),
    "nbdt_node_logits_backward": (c_int, [c_void_p, _P, c_int64, _P, _P]),
    "nbdt_hard_forward": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "nbdt_node_outputs": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "nbdt_tree_stats_accumulate": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P, _P, _P]),
    "nbdt_seg_pixel_fits": (c_int, [c_void_p]),
    "nbdt_seg_loss_workspace_floats": (c_int64, [c_int64, c_int64]),
    "nbdt_seg_soft_forward": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, c_int64, c_int64, _P, _P]),
    "nbdt_seg_soft_backward": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, c_int64, c_int64, _P, _P, _P]),
    "nbdt_seg_soft_tree_loss": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, c_int64, c_int64, _P, c_int64, c_float,
                                        c_float, c_float, c_float, _P, _P, _P, _P]),
    "nbdt_seg_hard_forward": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, c_int64, c_int64, _P, _P, _P]),
    "nbdt_seg_stats_fits": (c_int, [c_void_p]),
    "nbdt_seg_stats_accumulate": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, c_int64, c_int64, _P, c_int64, _P, _P, _P,
                                          _P, _P]),
    "nbdt_set_seg_stats_max_blocks": (c_int, [c_int]),
    "nbdt_get_seg_stats_max_blocks": (c_int, []),
    "nbdt_conv_igemm": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "nbdt_conv_pw": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "nbdt_conv_igemm_multi": (c_int, [_P, c_int32, _P, _P, _P, _P]),
    "nbdt_conv_igemm_stats": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, _P]),
    "nbdt_conv_seg_create": (c_int, [POINTER(ConvSegDesc), POINTER(c_void_p)]),
    "nbdt_conv_seg_destroy": (c_int, [c_void_p]),
    "nbdt_conv_seg_info": (c_int, [c_void_p, _I32P, _I32P, _I32P, _I32P, POINTER(c_int64)]),
    "nbdt_conv_seg_steps": (c_int, [c_void_p, c_int32, _I32P, c_int32, _I32P]),
    "nbdt_conv_seg_tile_weights": (c_int, [c_void_p, POINTER(c_void_p), _P, _P]),
    "nbdt_conv_seg": (c_int, [c_void_p, POINTER(c_void_p), _P, _P, _P, _P, _P]),
    "nbdt_ref_conv_seg": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), _P, _P, _P]),
    "nbdt_bn_apply_s2d": (c_int, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_bn_apply_s2d": (c_int, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_bn_finalize": (c_int, [c_int32, c_int32, c_int32, c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "nbdt_conv_igemm_bnbwd": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nbdt_conv_igemm_affine": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, c_int32, _P]),
    "nbdt_bn_bwd_fold": (c_int, [c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P]),
    "nbdt_bn_bwd_apply_cus": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, c_int32, _P]),
    "nbdt_bn_bwd_reduce_cus": (c_int, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, c_int32, _P]),
    "nbdt_bn_bwd_cus": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P,
                                c_int32, _P]),
    "nbdt_conv_wgrad": (c_int, [POINTER(WgradDesc), _P, _P, _P, _P]),
    "nbdt_ref_conv": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "nbdt_ref_wgrad": (c_int, [POINTER(WgradDesc), _P, _P, _P, _P]),
    "nbdt_conv_group_weight_prep": (c_int, [_P, c_int32, c_int32, _P, _P, _P]),
    "nbdt_conv_group_weight_prep_batched": (c_int, [_P, _P, c_int32, c_int64, _P, _P, _P]),
    "nbdt_conv_group_fwd": (c_int, [_P, _P, _P] + [c_int32] * 6 + [_P, _P, c_int32, _P]),
    "nbdt_conv_group_dgrad": (c_int, [_P, _P, _P] + [c_int32] * 7 + [_P]),
    "nbdt_conv_group_wgrad": (c_int, [_P, _P, _P] + [c_int32] * 6 + [_P]),
    "nbdt_ref_conv_group_fwd": (c_int, [_P, _P, _P] + [c_int32] * 6 + [_P]),
    "nbdt_ref_conv_group_dgrad": (c_int, [_P, _P, _P] + [c_int32] * 7 + [_P]),
    "nbdt_ref_conv_group_wgrad": (c_int, [_P, _P, _P] + [c_int32] * 6 + [_P]),
    "nbdt_ref_bn_stats": (c_int, [_P, c_int32, c_int32, c_int32, c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "nbdt_ref_bn_apply": (c_int, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_bn_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, _P, c_int32, c_int32, c_int32, c_int32,
                                c_int32, _P, _P, _P, _P, _P, _P]),
    "nbdt_ref_bn_relu_pool": (c_int, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_stem_conv": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_stem_wgrad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_bn_act_apply": (c_int, [_P, _P, _P, _P, _P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_bn_act_pool": (c_int, [_P, _P, _P, _P, _P, c_int32, _P, c_float, c_int32, c_int32, c_int32, c_int32, _P,
                                     _P]),
    "nbdt_ref_bn_act_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, _P, c_int32, c_int32, c_int32, c_int32, _P,
                                    _P, _P, _P, _P]),
    "nbdt_ref_bn_act_apply_rows": (c_int, [_P, _P, _P, _P, _P, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P,
                                           _P]),
    "nbdt_ref_bn_act_bwd_rows": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, _P, c_int32, c_int32, c_int32,
                                         c_int32, _P, _P, _P, _P, _P]),
    "nbdt_ref_dwconv_fwd": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_dwconv_bwd_data": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_dwconv_bwd_weight": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_weight_prep": (c_int, [_P, c_int32, c_int32, c_int32, _P, _P, _P]),
    "nbdt_weight_prep_batched": (c_int, [_P, _P, c_int32, c_int64, _P, _P]),
    "nbdt_weight_tile_batched": (c_int, [_P, _P, c_int32, c_int64, _P, _P]),
    "nbdt_bn_stats": (c_int, [_P, c_int32, c_int32, c_int32, c_int32, c_float, c_float, _P, _P, _P, _P, _P, _P]),
    "nbdt_bn_apply": (c_int, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_bn_bwd_reduce": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32,
                                   _P, _P, _P, _P, _P]),
    "nbdt_bn_bwd_apply": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32,
                                  c_int32, _P, _P, _P]),
    "nbdt_bn_relu_pool": (c_int, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_pool_bn_bwd_reduce": (c_int, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P,
                                        _P, _P, _P]),
    "nbdt_pool_bn_bwd_apply": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P,
                                       _P]),
    "nbdt_stem_conv": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_stem_wgrad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_bn_act_apply": (c_int, [_P, _P, _P, _P, _P, c_int32, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_bn_act_pool": (c_int, [_P, _P, _P, _P, _P, c_int32, _P, c_float, c_int32, c_int32, c_int32, c_int32,
                                 _P, _P]),
    "nbdt_bn_act_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int32, _P, c_int32, c_int32, c_int32, c_int32,
                                _P, _P, _P, _P, _P, _P]),
    "nbdt_dwconv_fwd": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P]),
    "nbdt_dwconv_bwd_data": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_dwconv_bwd_data_bn": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nbdt_bn_act_bwd_apply": (c_int, [_P, _P, _P, _P, _P, _P, c_int32, _P, c_int32, c_int32, c_int32, c_int32,
                                      _P, _P, _P, _P, _P, _P]),
    "nbdt_bn_act_se_sums": (c_int, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_bn_act_se_bwd_apply": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         _P, _P, _P, _P, _P]),
    "nbdt_dwconv_bwd_weight": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    # padded strided convolutions (nbdt_version() >= 126): (..., k | cpad, stride, pad_top, pad_left, ...)
    "nbdt_dwconv_fwd_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P]),
    "nbdt_dwconv_bwd_data_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_dwconv_bwd_weight_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_stem_conv_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_stem_wgrad_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_dwconv_fwd_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_dwconv_bwd_data_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_dwconv_bwd_weight_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_stem_conv_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_ref_stem_wgrad_pad": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_se_gate_fwd": (c_int, [_P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P]),
    "nbdt_se_gate_bwd": (c_int, [_P, _P, _P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P,
                                 _P, _P, _P]),
    "nbdt_se_param_grad": (c_int, [_P, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P]),
    "nbdt_dropout_fwd": (c_int, [_P, c_int64, c_float, ctypes.c_uint32, _P, _P, _P]),
    "nbdt_dropout_bwd": (c_int, [_P, c_int64, c_float, _P, _P, _P]),
    "nbdt_bn_act_apply_rows": (c_int, [_P, _P, _P, _P, _P, c_int32, _P, _P, _P, c_int32, c_int32, c_int32, c_int32, _P,
                                       _P]),
    "nbdt_bn_act_bwd_rows": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int32, _P, c_int32, c_int32, c_int32, c_int32,
                                     _P, _P, _P, _P, _P, _P]),
    "nbdt_stochastic_depth_draw": (c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, POINTER(c_float),
                                           POINTER(c_float), c_int32, c_int32, _P, _P]),
    "nbdt_augment_batch": (c_int, [_P, c_int32, _P, _P, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32,
                                   POINTER(c_float), POINTER(c_float), POINTER(c_float), ctypes.c_uint64, ctypes.c_uint64,
                                   _P, _P, _P, _P, _P]),
    "nbdt_resized_crop_batch": (c_int, [_P, c_int32, _P, _P, c_int32, c_int64] + [c_int32] * 9 +
                                [POINTER(c_float), POINTER(c_float), POINTER(ctypes.c_double), POINTER(ctypes.c_double), _P,
                                 ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P, _P, _P]),
    "nbdt_resized_crop_band_rows": (c_int, [c_int32] * 8),
    "nbdt_augment_batch_sharded": (c_int, [_P, c_int32, _P, _P, c_int64, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32,
                                           POINTER(c_float), POINTER(c_float), POINTER(c_float), ctypes.c_uint64,
                                           ctypes.c_uint64, _P, _P, _P, _P, _P]),
    "nbdt_resized_crop_batch_sharded": (c_int, [_P, c_int32, _P, _P, c_int64, c_int32, c_int64] + [c_int32] * 9 +
                                        [POINTER(c_float), POINTER(c_float), POINTER(ctypes.c_double),
                                         POINTER(ctypes.c_double), _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P, _P, _P]),
    "nbdt_policy_batch": (c_int, [_P, c_int32, _P, _P, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32,
                                  POINTER(c_float), POINTER(c_float), c_int32, _P, ctypes.c_double,
                                  POINTER(ctypes.c_double), POINTER(ctypes.c_double), _P, ctypes.c_uint64, ctypes.c_uint64,
                                  _P, _P, _P, _P, _P, _P, _P]),
    "nbdt_policy_batch_sharded": (c_int, [_P, c_int32, _P, _P, c_int64, c_int32, c_int64, c_int32, c_int32, c_int32,
                                          c_int32, POINTER(c_float), POINTER(c_float), c_int32, _P, ctypes.c_double,
                                          POINTER(ctypes.c_double), POINTER(ctypes.c_double), _P, ctypes.c_uint64,
                                          ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P]),
    "nbdt_policy_chain_batch": (c_int, [_P, c_int32, _P, _P, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32,
                                        POINTER(c_float), POINTER(c_float), c_int32, c_int32, _P, c_int32, c_int32, _P,
                                        c_int32, ctypes.c_double, POINTER(ctypes.c_double), POINTER(ctypes.c_double), _P,
                                        ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "nbdt_policy_chain_batch_sharded": (c_int, [_P, c_int32, _P, _P, c_int64, c_int32, c_int64, c_int32, c_int32, c_int32,
                                                c_int32, POINTER(c_float), POINTER(c_float), c_int32, c_int32, _P, c_int32,
                                                c_int32, _P, c_int32, ctypes.c_double, POINTER(ctypes.c_double),
                                                POINTER(ctypes.c_double), _P, ctypes.c_uint64, ctypes.c_uint64, _P, _P, _P,
                                                _P, _P, _P, _P, _P, _P]),
    "nbdt_resized_crop_policy_batch": (c_int, [_P, c_int32, _P, _P, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32,
                                               POINTER(c_float), POINTER(c_float), POINTER(ctypes.c_double),
                                               POINTER(ctypes.c_double), _P, c_int32, c_int32, _P, c_int32, c_int32, _P,
                                               c_int32, ctypes.c_double, POINTER(ctypes.c_double), POINTER(ctypes.c_double),
                                               _P, ctypes.c_uint64, ctypes.c_uint64] + [_P] * 11),
    "nbdt_resized_crop_policy_batch_sharded": (c_int, [_P, c_int32, _P, _P, c_int64, c_int32, c_int64, c_int32, c_int32,
                                                       c_int32, c_int32, POINTER(c_float), POINTER(c_float),
                                                       POINTER(ctypes.c_double), POINTER(ctypes.c_double), _P, c_int32,
                                                       c_int32, _P, c_int32, c_int32, _P, c_int32, ctypes.c_double,
                                                       POINTER(ctypes.c_double), POINTER(ctypes.c_double), _P,
                                                       ctypes.c_uint64, ctypes.c_uint64] + [_P] * 11),
    "nbdt_stem_patches": (c_int, [_P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_maxpool3x3s2_fwd": (c_int, [_P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P, _P]),
    "nbdt_maxpool3x3s2_bwd": (c_int, [_P, _P, c_int32, c_int32, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_linear_fwd": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P]),
    "nbdt_linear_bwd": (c_int, [_P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "nbdt_sgd_step": (c_int, [_P, _P, _P, c_int64, c_float, c_float, c_float, c_float, _P, c_int32, _P]),
    "nbdt_lars_create": (c_int, [c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_float), _I32P, c_int32,
                                 POINTER(c_void_p)]),
    "nbdt_lars_destroy": (c_int, [c_void_p]),
    "nbdt_lars_step": (c_int, [c_void_p, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, _P, c_int32, _P]),
    "nbdt_lars_ratios": (c_void_p, [c_void_p]),
    "nbdt_lars_ratios_to_host": (c_int, [c_void_p, POINTER(c_float), _P]),
    "nbdt_ema_update": (c_int, [_P, _P, c_int64, c_float, _P]),
    "nbdt_ema_update_multi": (c_int, [_P, c_int32, c_float, _P]),
    "nbdt_ema_swap": (c_int, [_P, _P, _P, c_int64, _P]),
    "nbdt_ema_swap_multi": (c_int, [_P, c_int32, _P]),
    "nbdt_arena_opt_create": (c_int, [c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_float), c_int32,
                                      POINTER(c_void_p)]),
    "nbdt_arena_opt_destroy": (c_int, [c_void_p]),
    "nbdt_arena_opt_n": (c_int64, [c_void_p]),
    "nbdt_adamw_step": (c_int, [c_void_p, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_int64, c_float, _P,
                                c_int32, _P]),
    "nbdt_rmsprop_step": (c_int, [c_void_p, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_int32, c_float, _P,
                                  c_int32, _P]),
    "nbdt_clip_create": (c_int, [c_int64, POINTER(c_void_p)]),
    "nbdt_clip_destroy": (c_int, [c_void_p]),
    "nbdt_clip_norm": (c_int, [c_void_p, _P, c_float, c_float, _P]),
    "nbdt_clip_apply": (c_int, [c_void_p, _P, _P]),
    "nbdt_clip_record": (c_void_p, [c_void_p]),
    "nbdt_clip_record_to_host": (c_int, [c_void_p, _P, _P]),
    # agglomerative clustering (nbdt_version() >= 128): (centers, n, d, method, metric, workspace, workspace_bytes, ...)
    "nbdt_linkage_workspace_bytes": (c_int, [c_int64, POINTER(c_int64)]),
    "nbdt_linkage": (c_int, [_P, c_int64, c_int64, c_int32, c_int32, _P, c_int64, _P, _P, _P, _P]),
    # superclass evaluation (nbdt_version() >= 131): (groups, z, ztype, B, ldz, ...)
    "nbdt_groups_create": (c_int, [c_int, c_int, c_int, _I32P, _I32P, POINTER(c_void_p)]),
    "nbdt_groups_destroy": (c_int, [c_void_p]),
    "nbdt_group_logits": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P]),
    "nbdt_group_logits_backward": (c_int, [c_void_p, _P, c_int64, _P, _P]),
    "nbdt_superclass_accumulate": (c_int, [c_void_p, _P, c_int, c_int64, c_int64, _P, _P, c_int32, _P, c_int32, _P, _P,
                                           _P, _P]),
    # cross-entropy on upsampled logits (nbdt_version() >= 133): (x, xtype, N, C, h, w, xi, xc, y, H, W, align_corners,
    # ignore_index, weight, smoothing, grad_scale, workspace, loss, gx, stream)
    "nbdt_upsample_taps": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_float),
                                   POINTER(c_float)]),
    "nbdt_upsample_footprint": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    "nbdt_upsampled_xent_workspace_floats": (c_int64, [c_int64, c_int64, c_int64]),
    "nbdt_upsampled_xent": (c_int, [_P, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, _P, c_int64, c_int64,
                                    c_int, c_int64, _P, c_float, c_float, _P, _P, _P, _P]),
}


def _missing(name):
    def raiser(*_a, **_k):
        raise NBDTHipError(f"{_LIBPATH} does not export {name}: stale build, re-run build()")
    return raiser


def exported_symbols():
    """Names from SIGNATURES the loaded library really exports (used by the C-ABI test)."""
    l = ctypes.CDLL(_LIBPATH)
    return [n for n in SIGNATURES if hasattr(l, n)]


def lib():
    """Load the shared library (once).  Raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise NBDTHipError(
                f"{_LIBPATH} is missing: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the NBDT hot path.")
        l = ctypes.CDLL(_LIBPATH)
        # a timing build (csrc/common.h: -DNBDT_TIMING_BUILD + a switch that stamps a kernel's segments with s_memtime)
        # is slower and exports debug globals: only the measurement scripts under scratch/ may load one
        if hasattr(l, "nbdt_timing_build") and os.environ.get("NBDT_ALLOW_TIMING_BUILD") != "1":
            raise NBDTHipError(f"{_LIBPATH} is a timing build (exports nbdt_timing_build): its kernels carry "
                               "stamp instrumentation.  Set NBDT_ALLOW_TIMING_BUILD=1 in a measurement script; never train with it.")
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                setattr(l, name, _missing(name))  # stale .so: fail loudly on first use
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def libpath():
    return _LIBPATH


def check(rc):
    if rc != 0:
        raise NBDTHipError(f"libnbdt_hip error {rc}: {lib().nbdt_last_error().decode()}")


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def stream_of(t):
    return c_void_p(_raw_stream(t.device.index))      # = torch.cuda.current_stream(t.device).cuda_stream, without the Stream object


def require_gpu(t, what):
    if not t.is_cuda:
        raise NBDTHipError(
            f"{what}: tensor is on {t.device}; the NBDT hot path runs on MI355X only "
            "(no CPU fallback -- move inputs to a HIP device)")


def ztype_of(t):
    try:
        return _ZTYPE[t.dtype]
    except KeyError:
        raise NBDTHipError(f"unsupported logits dtype {t.dtype}") from None


class TreeHandle:
    """Owns one nbdt_tree on one device."""

    def __init__(self, flat, device_index):
        self.flat = flat
        self.device_index = device_index
        out = c_void_p()
        as_p = lambda a: a.ctypes.data_as(_I32P)
        check(lib().nbdt_tree_create(
            int(device_index), flat.num_classes, flat.num_inodes, flat.root,
            as_p(flat.node_off), as_p(flat.slot_off), as_p(flat.slot_cls),
            as_p(flat.cls_off), as_p(flat.cls_slot), as_p(flat.slot_next), ctypes.byref(out)))
        self.h = out
        self.max_depth = lib().nbdt_tree_max_depth(self.h)

    def __del__(self):
        try:
            if getattr(self, "h", None) and _lib is not None:
                _lib.nbdt_tree_destroy(self.h)
        except Exception:
            pass


def last_rules_path():
    """Which form the calling thread's last rules launch took: "lds", "lds-unstaged" or "global" ("" before the first)."""
    return lib().nbdt_debug_last_rules_path().decode()


def _rows(z, handle):
    """[B, C] tensor with unit column stride -> (tensor, B, ldz).  C must be the hierarchy's class count: the
    kernels index columns by class, so wider logits would be silently truncated and narrower ones over-read."""
    if z.dim() != 2:
        raise NBDTHipError(f"rules layer expects [B, C] logits, got shape {tuple(z.shape)}")
    if z.shape[1] != handle.flat.num_classes:
        raise NBDTHipError(f"logits have {z.shape[1]} columns but the hierarchy has {handle.flat.num_classes} classes")
    if z.stride(1) != 1 or (z.shape[0] > 1 and z.stride(0) < z.shape[1]):
        z = z.contiguous()
    return z, z.shape[0], (z.stride(0) if z.shape[0] > 1 else z.shape[1])


def _class_targets(y, z):
    if y.is_floating_point() or y.dim() != 1:
        raise NBDTHipError("the fused tree losses take class-index targets [B]; soft / probability targets go "
                           "through the composed path (pass a criterion that is not a default CrossEntropyLoss)")
    return y.to(device=z.device, dtype=torch.int64).contiguous()


def soft_forward(handle, z):
    require_gpu(z, "soft_forward")
    handle.flat.require_single_path()
    z, B, ld = _rows(z, handle)
    P = torch.empty((B, handle.flat.num_classes), dtype=torch.float32, device=z.device)
    check(lib().nbdt_soft_forward(handle.h, ptr(z), ztype_of(z), B, ld, ptr(P), stream_of(z)))
    return P


def soft_backward(handle, z, gP):
    require_gpu(z, "soft_backward")
    handle.flat.require_single_path()
    z, B, ld = _rows(z, handle)
    gP = gP.contiguous().float()
    gz = torch.empty((B, handle.flat.num_classes), dtype=torch.float32, device=z.device)
    check(lib().nbdt_soft_backward(handle.h, ptr(z), ztype_of(z), B, ld, ptr(gP), ptr(gz), stream_of(z)))
    return gz


def _soft_tree_loss_ex(handle, z, B, ld, y, t, ldt, smoothing, w_xent, w_tree, grad_scale):
    row = torch.empty((B,), dtype=torch.float32, device=z.device)
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    gz = torch.empty((B, handle.flat.num_classes), dtype=torch.float32, device=z.device)
    check(lib().nbdt_soft_tree_loss_ex(handle.h, ptr(z), ztype_of(z), B, ld, ptr(y), ptr(t), int(ldt), float(smoothing),
                                       float(w_xent), float(w_tree), float(grad_scale), ptr(row), ptr(loss), ptr(gz),
                                       stream_of(z)))
    return loss, gz


def soft_tree_loss(handle, z, y, w_xent, w_tree, grad_scale=1.0, smoothing=0.0):
    """Returns (loss scalar tensor, gz [B,C] fp32).  smoothing: the criterion's label_smoothing (nbdt_soft_tree_loss_ex)."""
    require_gpu(z, "soft_tree_loss")
    handle.flat.require_single_path()
    z, B, ld = _rows(z, handle)
    y = _class_targets(y, z)
    return _soft_tree_loss_ex(handle, z, B, ld, y, None, 0, smoothing, w_xent, w_tree, grad_scale)


def soft_tree_loss_dense(handle, z, t, w_xent, w_tree, grad_scale=1.0, smoothing=0.0):
    """The same loss on probability targets t [B, C] fp32 (MixUp / CutMix, soft labels): (loss, gz [B,C] fp32).  The rows
    are used as given -- not normalised, like torch's criterion."""
    require_gpu(z, "soft_tree_loss_dense")
    handle.flat.require_single_path()
    z, B, ld = _rows(z, handle)
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != tuple(z.shape):
        raise NBDTHipError(f"probability targets must be fp32 [B, C] = {tuple(z.shape)}, got "
                           f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if t.device != z.device:
        raise NBDTHipError(f"probability targets are on {t.device}, the logits on {z.device}")
    if t.stride(1) != 1 or (B > 1 and t.stride(0) < t.shape[1]):
        raise NBDTHipError(f"probability targets need unit column stride and non-overlapping rows, got strides {t.stride()}")
    ldt = t.stride(0) if B > 1 else t.shape[1]
    return _soft_tree_loss_ex(handle, z, B, ld, None, t, ldt, smoothing, w_xent, w_tree, grad_scale)


def head_soft_tree_loss(handle, pooled, W, bias, y, w_xent, w_tree, grad_scale=1.0, gW=None, gb=None,
                        want_logits=False, want_gpooled=True):
    """Classifier head + SoftTreeSupLoss forward and backward in ONE launch (nbdt_head_soft_tree_loss): returns
    (loss, dL/dpooled or None, logits or None); dL/dW and dL/db are ACCUMULATED into gW / gb when given."""
    require_gpu(pooled, "head_soft_tree_loss")
    handle.flat.require_single_path()
    if pooled.dtype != torch.float32 or W.dtype != torch.float32 or not pooled.is_contiguous() or not W.is_contiguous():
        raise NBDTHipError("head_soft_tree_loss takes contiguous fp32 features [B, K] and weights [C, K]")
    B, K = pooled.shape
    C = handle.flat.num_classes
    if tuple(W.shape) != (C, K):
        raise NBDTHipError(f"classifier weight is {tuple(W.shape)}, the hierarchy has {C} classes over {K} features")
    y = _class_targets(y, pooled)
    row = torch.empty((B,), dtype=torch.float32, device=pooled.device)
    loss = torch.empty((), dtype=torch.float32, device=pooled.device)
    z = torch.empty((B, C), dtype=torch.float32, device=pooled.device) if want_logits else None
    gp = torch.empty((B, K), dtype=torch.float32, device=pooled.device) if want_gpooled else None
    check(lib().nbdt_head_soft_tree_loss(handle.h, ptr(pooled), ptr(W), ptr(bias), B, K, ptr(y), float(w_xent),
                                         float(w_tree), float(grad_scale), ptr(row), ptr(loss), ptr(z), ptr(gp),
                                         ptr(gW), ptr(gb), stream_of(pooled)))
    return loss, gp, z


def hard_tree_loss(handle, z, y, w_xent, w_node, grad_scale=1.0, smoothing=0.0):
    """HardTreeSupLoss fused: returns (loss scalar tensor, gz [B,C] fp32).  smoothing: the criterion's label_smoothing."""
    require_gpu(z, "hard_tree_loss")
    z, B, ld = _rows(z, handle)
    y = _class_targets(y, z)
    row = torch.empty((B,), dtype=torch.float32, device=z.device)
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    gz = torch.empty((B, handle.flat.num_classes), dtype=torch.float32, device=z.device)
    check(lib().nbdt_hard_tree_loss_ex(handle.h, ptr(z), ztype_of(z), B, ld, ptr(y), float(smoothing), float(w_xent),
                                       float(w_node), float(grad_scale), ptr(row), ptr(loss), ptr(gz),
                                       stream_of(z)))
    return loss, gz


def node_logits(handle, z):
    """[B, R] fp32 child logits of every inner node (slot-major)."""
    require_gpu(z, "node_logits")
    z, B, ld = _rows(z, handle)
    logits = torch.empty((B, handle.flat.num_slots), dtype=torch.float32, device=z.device)
    check(lib().nbdt_node_outputs(handle.h, ptr(z), ztype_of(z), B, ld, ptr(logits), None, None, None,
                                  stream_of(z)))
    return logits


def node_logits_backward(handle, gs):
    require_gpu(gs, "node_logits_backward")
    gs = gs.contiguous().float()
    gz = torch.empty((gs.shape[0], handle.flat.num_classes), dtype=torch.float32, device=gs.device)
    check(lib().nbdt_node_logits_backward(handle.h, ptr(gs), gs.shape[0], ptr(gz), stream_of(gs)))
    return gz


def hard_forward(handle, z, want_onehot=True, want_decisions=False):
    require_gpu(z, "hard_forward")
    z, B, ld = _rows(z, handle)
    C, D = handle.flat.num_classes, handle.max_depth
    dev = z.device
    pred = torch.empty((B,), dtype=torch.int64, device=dev)
    onehot = torch.empty((B, C), dtype=torch.float32, device=dev) if want_onehot else None
    if want_decisions:
        pn = torch.empty((B, D), dtype=torch.int32, device=dev)
        pc = torch.empty((B, D), dtype=torch.int32, device=dev)
        pp = torch.empty((B, D), dtype=torch.float32, device=dev)
        pe = torch.empty((B, D), dtype=torch.float32, device=dev)
    else:
        pn = pc = pp = pe = None
    check(lib().nbdt_hard_forward(handle.h, ptr(z), ztype_of(z), B, ld, ptr(pred), ptr(onehot), ptr(pn),
                                  ptr(pc), ptr(pp), ptr(pe), stream_of(z)))
    return pred, onehot, (pn, pc, pp, pe)


def node_outputs(handle, z):
    require_gpu(z, "node_outputs")
    z, B, ld = _rows(z, handle)
    R, N = handle.flat.num_slots, handle.flat.num_inodes
    dev = z.device
    logits = torch.empty((B, R), dtype=torch.float32, device=dev)
    probs = torch.empty((B, R), dtype=torch.float32, device=dev)
    preds = torch.empty((B, N), dtype=torch.int64, device=dev)
    ent = torch.empty((B, N), dtype=torch.float32, device=dev)
    check(lib().nbdt_node_outputs(handle.h, ptr(z), ztype_of(z), B, ld, ptr(logits), ptr(probs),
                                  ptr(preds), ptr(ent), stream_of(z)))
    return logits, probs, preds, ent


# ---------------------------------------------------------------------------------------------------------------
# ad-hoc class groupings and superclass evaluation: csrc/superclass.hip

NBDT_SUPER_MASKED, NBDT_SUPER_GROUP_MEAN = 0, 1


class GroupsHandle:
    """Owns one nbdt_groups on one device.  groups: a sequence of G class-index sequences (the order of each is the
    order its sum runs in) over num_classes classes."""

    def __init__(self, groups, num_classes, device_index):
        self.groups = tuple(tuple(int(c) for c in g) for g in groups)
        self.num_classes, self.num_groups, self.device_index = int(num_classes), len(self.groups), device_index
        off = np.zeros(self.num_groups + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(g) for g in self.groups])
        cls = np.array([c for g in self.groups for c in g] or [0], dtype=np.int32)
        out = c_void_p()
        check(lib().nbdt_groups_create(int(device_index), self.num_classes, self.num_groups, off.ctypes.data_as(_I32P),
                                       cls.ctypes.data_as(_I32P), ctypes.byref(out)))
        self.h = out

    def __del__(self):
        try:
            if getattr(self, "h", None) and _lib is not None:
                _lib.nbdt_groups_destroy(self.h)
        except Exception:
            pass


_groups_cache = {}
GROUPS_CACHE_MAX = 64       # handles kept: a caller that keeps inventing groupings must not pin device memory for good


def groups_handle(groups, num_classes, device_index):
    """The cached handle of one (grouping, class count, device), the way a Tree caches its handle per device.  The cache
    holds the GROUPS_CACHE_MAX most recently used handles; one that falls out is destroyed when its last user (an
    analyzer, an autograd graph) lets go of it."""
    key = (tuple(tuple(int(c) for c in g) for g in groups), int(num_classes), device_index)
    h = _groups_cache.pop(key, None)
    if h is None:
        h = GroupsHandle(key[0], num_classes, device_index)
    _groups_cache[key] = h              # (re)inserted last: dicts keep insertion order, the first key is the oldest
    while len(_groups_cache) > GROUPS_CACHE_MAX:
        del _groups_cache[next(iter(_groups_cache))]
    return h


def _group_rows(z, handle):
    if z.dim() != 2:
        raise NBDTHipError(f"group logits expect [B, C] logits, got shape {tuple(z.shape)}")
    if z.shape[1] != handle.num_classes:
        raise NBDTHipError(f"logits have {z.shape[1]} columns but the grouping is over {handle.num_classes} classes")
    if z.stride(1) != 1 or (z.shape[0] > 1 and z.stride(0) < z.shape[1]):
        z = z.contiguous()
    return z, z.shape[0], (z.stride(0) if z.shape[0] > 1 else z.shape[1])


def group_logits(handle, z):
    """[B, G] fp32: the mean of the logits of every group's classes (nbdt_group_logits)."""
    require_gpu(z, "group_logits")
    z, B, ld = _group_rows(z, handle)
    out = torch.empty((B, handle.num_groups), dtype=torch.float32, device=z.device)
    check(lib().nbdt_group_logits(handle.h, ptr(z), ztype_of(z), B, ld, ptr(out), stream_of(z)))
    return out


def group_logits_backward(handle, gs):
    require_gpu(gs, "group_logits_backward")
    gs = gs.contiguous().float()
    gz = torch.empty((gs.shape[0], handle.num_classes), dtype=torch.float32, device=gs.device)
    check(lib().nbdt_group_logits_backward(handle.h, ptr(gs), gs.shape[0], ptr(gz), stream_of(gs)))
    return gz


def superclass_accumulate(handle, z, y, map_target, map_pred, mode, totals, confusion=None, want_pred=False):
    """One evaluation batch added into the int64 device counters totals [2] and confusion [G, G] (nullable) by ONE launch
    (nbdt_superclass_accumulate); nothing here waits for the GPU.  map_target / map_pred: int32 device tensors.  Returns
    the predicted superclass of every row [B] int64 when want_pred, else None."""
    require_gpu(z, "superclass_accumulate")
    z, B, ld = _group_rows(z, handle)
    for name, t, dt in (("targets", y, torch.int64), ("map_target", map_target, torch.int32),
                        ("map_pred", map_pred, torch.int32), ("totals", totals, torch.int64),
                        ("confusion", confusion, torch.int64)):
        if t is None and name in ("map_pred", "confusion"):
            continue
        if t.dtype != dt or t.device != z.device or not t.is_contiguous():
            raise NBDTHipError(f"superclass_accumulate: {name} must be a contiguous {dt} tensor on {z.device}, got "
                               f"{t.dtype} on {t.device}")
    if y.shape != (B,):
        raise NBDTHipError(f"superclass_accumulate: {B} rows of logits but targets of shape {tuple(y.shape)}")
    if map_pred is not None and map_pred.numel() != handle.num_classes:
        raise NBDTHipError(f"map_pred has {map_pred.numel()} entries, the grouping is over {handle.num_classes} classes")
    G = handle.num_groups
    if totals.numel() != 2 or (confusion is not None and confusion.numel() != G * G):
        raise NBDTHipError(f"superclass_accumulate: totals must hold 2 counters and confusion {G} x {G}")
    pred = torch.empty((B,), dtype=torch.int64, device=z.device) if want_pred else None
    check(lib().nbdt_superclass_accumulate(handle.h, ptr(z), ztype_of(z), B, ld, ptr(y), ptr(map_target),
                                           int(map_target.numel()), ptr(map_pred), int(mode), ptr(totals),
                                           ptr(confusion), ptr(pred), stream_of(z)))
    return pred


# ---------------------------------------------------------------------------------------------------------------
# the rules on NCHW logits (segmentation): csrc/rules_pixel.h, one lane per pixel

SEG_PIXEL_MAX_ROWS = 640      # kPixMaxRows: child slots + largest fan-out, at 64 lanes x 4 bytes each within 160 KB of LDS


def seg_pixel_fits(flat):
    """The pixel form's size limit (include/nbdt_hip.h, nbdt_seg_*): R + F <= 640 -- a pure function of the hierarchy."""
    fan = int((flat.node_off[1:] - flat.node_off[:-1]).max())
    on_a_path = bool((flat.cls_off[1:] > flat.cls_off[:-1]).all())      # a class under no child has no chain to walk
    return on_a_path and flat.num_slots + fan <= SEG_PIXEL_MAX_ROWS


def _dense_planes(shape, strides):
    """[N, C, H, W] whose planes are contiguous over pixels and do not overlap (a channel-sliced view qualifies)."""
    (N, C, H, W), (sn, sc, sh, sw) = shape, strides
    return ((W == 1 or sw == 1) and (H == 1 or sh == W) and (C == 1 or sc >= H * W)
            and (N == 1 or sn >= (C - 1) * (sc if C > 1 else 0) + H * W))


def _pixel_rows(shape, strides):
    """[N, C, H, W] whose memory is already [N*H*W, C] rows of unit column stride (channels_last)."""
    (N, C, H, W), (sn, sc, sh, sw) = shape, strides
    ld = sw if W > 1 else (sh if H > 1 else (sn if N > 1 else C))
    return ((C == 1 or sc == 1) and ld >= C and (W == 1 or sw == ld) and (H == 1 or sh == W * ld)
            and (N == 1 or sn == H * W * ld))


def seg_dispatch(shape, strides, dtype, flat):
    """Which way 4-D logits take through the rules -- a pure host function of (shape, strides, dtype, hierarchy):
      "pixel"       contiguous NCHW planes: the pixel kernels, as they are
      "rows"        channels_last memory is already [N*H*W, C] rows: the row kernels with ldz = C, no copy
      "contiguous"  anything else: one .contiguous(), then the pixel kernels
      "coerced"     a hierarchy beyond the pixel form's limit: the row kernels on one channels_last copy
    """
    if len(shape) != 4:
        raise NBDTHipError(f"segmentation rules expect [N, C, H, W] logits, got shape {tuple(shape)}")
    if shape[1] != flat.num_classes:
        raise NBDTHipError(f"logits have {shape[1]} channels but the hierarchy has {flat.num_classes} classes")
    if dtype not in _ZTYPE:
        raise NBDTHipError(f"unsupported logits dtype {dtype}")
    if _pixel_rows(shape, strides) and not (_dense_planes(shape, strides) and seg_pixel_fits(flat)):
        return "rows"
    if not seg_pixel_fits(flat):
        return "coerced"
    return "pixel" if _dense_planes(shape, strides) else "contiguous"


# ---- segmentation evaluation (nbdt_seg_stats_accumulate, csrc/seg_stats.h): the same layouts, one more limit

LDS_BYTES = 160 * 1024        # kLdsBytes


def flat_max_depth(flat):
    """Inner nodes on the longest walk from the root: nbdt_tree_max_depth, on the host."""
    children = lambda n: [int(v) for v in flat.slot_next[flat.node_off[n]:flat.node_off[n + 1]] if v >= 0]  # noqa: E731
    depth, stack = {}, [(int(flat.root), False)]
    while stack:
        n, done = stack.pop()
        if done:
            depth[n] = 1 + max((depth.get(m, 0) for m in children(n)), default=0)
        elif n not in depth:
            depth[n] = 0                 # (a cycle is refused by nbdt_tree_create; it must not loop for ever here)
            stack.append((n, True))
            stack.extend((m, False) for m in children(n) if m not in depth)
    return depth[int(flat.root)]


def seg_stats_lds_bytes(flat):
    """LDS of one block of the statistics kernel: the pixel form's (R + F) rows of 64 floats plus the block's int32
    counters [5 N][4 totals][max_depth + 1], padded to an even count."""
    fan = int((flat.node_off[1:] - flat.node_off[:-1]).max())
    small = (5 * int(flat.num_inodes) + 4 + flat_max_depth(flat) + 1 + 1) & ~1
    return (int(flat.num_slots) + fan) * 256 + 4 * small


def seg_stats_fits(flat):
    """nbdt_seg_stats_fits as a pure function of the hierarchy: the pixel form's limit and rows + counters <= 160 KB."""
    return seg_pixel_fits(flat) and seg_stats_lds_bytes(flat) <= LDS_BYTES


def _slot_schedule_len(slot_off, lanes):
    """sched_len of build_slot_schedule (csrc/rules.hip): passes of the busiest wave times the group's lanes."""
    R = len(slot_off) - 1
    length = np.diff(np.asarray(slot_off, dtype=np.int64))
    order = np.argsort(-length, kind="stable")
    waves, load, count = lanes // 64, [0] * (lanes // 64), [0] * (lanes // 64)
    for c in range((R + 63) // 64):
        w = min(range(waves), key=lambda i: (load[i], i))
        count[w] += 1
        load[w] += 64 + 8 * int(length[order[c * 64]])
    return max(count) * lanes


def tree_stats_fits(flat):
    """The limit of the row diagnostics (nbdt_tree_stats_accumulate: offset arrays, block counters and the unstaged
    sample rows of a block within 160 KB of LDS) as a pure function of the hierarchy."""
    C, N, R = int(flat.num_classes), int(flat.num_inodes), int(flat.num_slots)
    tps = 64 if (C <= 64 and R <= 64) else 256 if (C <= 512 and R <= 512) else 1024
    spb = max(tps, 256) // tps
    tl = ((N + 1) + (R + 1) + (C + 1) + 3 * _slot_schedule_len(flat.slot_off, tps) + 3) & ~3
    small = (5 * N + 4 + flat_max_depth(flat) + 1 + 1) & ~1
    tl += (small + 4 * N + 3) & ~3
    return (tl + spb * (C + 2 * R + 2 * N + 32) + 4) * 4 <= LDS_BYTES


def seg_stats_dispatch(shape, strides, dtype, flat):
    """Which way 4-D logits take through the segmentation statistics -- a pure host function like seg_dispatch:
      "pixel"       contiguous NCHW planes, hierarchy within nbdt_seg_stats_fits: nbdt_seg_stats_accumulate as it is
      "rows"        channels_last memory: nbdt_tree_stats_accumulate with ldz = C on the [N*H*W, C] view, no copy
      "contiguous"  other strides: one .contiguous(), then "pixel"
      "coerced"     beyond the pixel limit but within the row diagnostics': the rows of one channels_last copy
    and an error that names both limits beyond both."""
    if len(shape) != 4:
        raise NBDTHipError(f"segmentation statistics expect [N, C, H, W] logits, got shape {tuple(shape)}")
    if shape[1] != flat.num_classes:
        raise NBDTHipError(f"logits have {shape[1]} channels but the hierarchy has {flat.num_classes} classes")
    if dtype not in _ZTYPE:
        raise NBDTHipError(f"unsupported logits dtype {dtype}")
    limits = getattr(flat, "_seg_stats_limits", None)          # a function of the hierarchy alone: worked out once
    if limits is None:
        limits = (seg_stats_fits(flat), tree_stats_fits(flat))
        try:
            flat._seg_stats_limits = limits
        except AttributeError:
            pass
    pixel, rows = limits
    if not pixel and not rows:
        raise NBDTHipError(
            f"hierarchy too large for the segmentation statistics: the pixel form needs {seg_stats_lds_bytes(flat)} bytes "
            f"of LDS (rows (R + F) * 256 plus the block's counters; R + F <= {SEG_PIXEL_MAX_ROWS}) and the row diagnostics "
            f"(nbdt_tree_stats_accumulate) do not fit their sample rows either; both are limited to {LDS_BYTES} bytes")
    if rows and _pixel_rows(shape, strides) and not (_dense_planes(shape, strides) and pixel):
        return "rows"
    if not pixel:
        return "coerced"
    return "pixel" if _dense_planes(shape, strides) else "contiguous"


def _seg_route(z, handle):
    """-> ("pixel", z with dense planes) or ("rows", the [N*H*W, C] view of channels_last memory)."""
    how = seg_dispatch(tuple(z.shape), tuple(z.stride()), z.dtype, handle.flat)
    if how == "contiguous":
        z, how = z.contiguous(), "pixel"
    elif how == "coerced":
        z, how = z.contiguous(memory_format=torch.channels_last), "rows"
    if how == "rows":
        return how, z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    return how, z


def _seg_geom(z):
    N, C, H, W = z.shape
    zc = z.stride(1) if C > 1 else H * W
    zi = z.stride(0) if N > 1 else max(C - 1, 0) * zc + H * W
    return N, H * W, zi, zc


def _rows_to_nchw(rows, shape):
    """[N*H*W, K] -> [N, K, H, W] (a channels_last-strided view, no copy)."""
    N, _, H, W = shape
    return rows.view(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def seg_soft_forward(handle, z):
    """P [N, C, H, W] fp32 path probabilities of NCHW logits."""
    require_gpu(z, "seg_soft_forward")
    handle.flat.require_single_path()
    how, zz = _seg_route(z, handle)
    if how == "rows":
        return _rows_to_nchw(soft_forward(handle, zz), z.shape)
    N, HW, zi, zc = _seg_geom(zz)
    P = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device)
    check(lib().nbdt_seg_soft_forward(handle.h, ptr(zz), ztype_of(zz), N, HW, zi, zc, ptr(P), stream_of(zz)))
    return P


def seg_soft_backward(handle, z, gP):
    """gz [N, C, H, W] fp32 = d<gP, P>/dz, the forward recomputed from z."""
    require_gpu(z, "seg_soft_backward")
    handle.flat.require_single_path()
    how, zz = _seg_route(z, handle)
    if how == "rows":
        g = gP.float().permute(0, 2, 3, 1).reshape(-1, z.shape[1])
        return _rows_to_nchw(soft_backward(handle, zz, g), z.shape)
    N, HW, zi, zc = _seg_geom(zz)
    gP = gP.float().contiguous()
    gz = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device)
    check(lib().nbdt_seg_soft_backward(handle.h, ptr(zz), ztype_of(zz), N, HW, zi, zc, ptr(gP), ptr(gz), stream_of(zz)))
    return gz


def seg_soft_tree_loss(handle, z, y, ignore_index, w_xent, w_tree, grad_scale=1.0, smoothing=0.0):
    """SoftSegTreeSupLoss for nn.CrossEntropyLoss(ignore_index, label_smoothing=smoothing): (loss, gz [N, C, H, W] fp32),
    both means over the pixels with y != ignore_index; gz is 0 at the others."""
    require_gpu(z, "seg_soft_tree_loss")
    handle.flat.require_single_path()
    if y.is_floating_point() or y.dim() != 3 or (y.shape[0],) + tuple(y.shape[1:]) != (z.shape[0],) + tuple(z.shape[2:]):
        raise NBDTHipError(f"segmentation targets must be class indices [N, H, W] = "
                           f"{(z.shape[0],) + tuple(z.shape[2:])}, got {y.dtype} {tuple(y.shape)}")
    y = y.to(device=z.device, dtype=torch.int64).contiguous()
    how, zz = _seg_route(z, handle)
    if how == "rows":
        # the row losses take no ignore_index: they run on the valid rows alone (their mean is the mean over those)
        keep = (y.reshape(-1) != ignore_index).nonzero().squeeze(1)
        gz = torch.zeros((zz.shape[0], zz.shape[1]), dtype=torch.float32, device=z.device)
        if keep.numel() == 0:
            return torch.full((), float("nan"), dtype=torch.float32, device=z.device), _rows_to_nchw(gz, z.shape)
        loss, g = soft_tree_loss(handle, zz[keep], y.reshape(-1)[keep], w_xent, w_tree, grad_scale, smoothing)
        gz[keep] = g
        return loss, _rows_to_nchw(gz, z.shape)
    N, HW, zi, zc = _seg_geom(zz)
    ws = torch.empty((int(lib().nbdt_seg_loss_workspace_floats(N, HW)),), dtype=torch.float32, device=z.device)
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    gz = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device)
    check(lib().nbdt_seg_soft_tree_loss(handle.h, ptr(zz), ztype_of(zz), N, HW, zi, zc, ptr(y), int(ignore_index),
                                        float(smoothing), float(w_xent), float(w_tree), float(grad_scale), ptr(ws),
                                        ptr(loss), ptr(gz), stream_of(zz)))
    return loss, gz


def seg_hard_forward(handle, z, want_onehot=True):
    """(pred [N, H, W] int64, onehot [N, C, H, W] fp32 or None) of NCHW logits."""
    require_gpu(z, "seg_hard_forward")
    how, zz = _seg_route(z, handle)
    N, C, H, W = z.shape
    if how == "rows":
        pred, onehot, _ = hard_forward(handle, zz, want_onehot=want_onehot)
        return pred.view(N, H, W), (_rows_to_nchw(onehot, z.shape) if want_onehot else None)
    N, HW, zi, zc = _seg_geom(zz)
    pred = torch.empty((N, H, W), dtype=torch.int64, device=z.device)
    onehot = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device) if want_onehot else None
    check(lib().nbdt_seg_hard_forward(handle.h, ptr(zz), ztype_of(zz), N, HW, zi, zc, ptr(pred), ptr(onehot),
                                      stream_of(zz)))
    return pred, onehot


# ---- cross-entropy on bilinearly upsampled logits (nbdt_upsampled_xent, csrc/upsampled_xent.hip)

UPSAMPLE_MAX_EXTENT = 1 << 22       # kUpMaxExtent: H, W (the source index is an fp32)
UPSAMPLE_MAX_CLASSES = 4 * 65535    # kUpBwdC classes per grid.y block of the backward


def upsample_taps(n_in, n_out, align_corners, dst):
    """(i0, i1, l0, l1) of destination index dst on an axis of n_in source and n_out destination samples: what the
    kernels use, from their own function (no device involved)."""
    i0, i1, l0, l1 = c_int(), c_int(), c_float(), c_float()
    check(lib().nbdt_upsample_taps(int(n_in), int(n_out), int(bool(align_corners)), int(dst), ctypes.byref(i0),
                                   ctypes.byref(i1), ctypes.byref(l0), ctypes.byref(l1)))
    return i0.value, i1.value, l0.value, l1.value


def upsample_footprint(n_in, n_out, align_corners, i):
    """(lo, hi): the inclusive range of destinations whose taps can touch source index i (no device involved)."""
    lo, hi = c_int(), c_int()
    check(lib().nbdt_upsample_footprint(int(n_in), int(n_out), int(bool(align_corners)), int(i), ctypes.byref(lo),
                                        ctypes.byref(hi)))
    return lo.value, hi.value


def upsampled_xent_refusal(shape, dtype, target_shape, target_dtype, has_weight, smoothing):
    """Why nbdt_upsampled_xent does not take this call, or None -- a pure host function of shapes, dtypes and the
    criterion's settings (the entry's own refusals, ahead of any allocation)."""
    if len(shape) != 4 or len(target_shape) != 3:
        return f"logits {tuple(shape)} / targets {tuple(target_shape)} are not [N, C, h, w] / [N, H, W]"
    if dtype not in _ZTYPE:
        return f"unsupported logits dtype {dtype}"
    if target_dtype.is_floating_point or target_dtype in (torch.bool, torch.complex64, torch.complex128):
        return f"targets of type {target_dtype} are not class indices"
    (N, C, h, w), (Ny, H, W) = shape, target_shape
    if Ny != N:
        return f"{Ny} target images for {N} logit images"
    if min(N, C, h, w) <= 0:
        return "empty tensor"
    if H < h or W < w:
        return f"downsampling ({h} x {w} -> {H} x {W})"
    if H > UPSAMPLE_MAX_EXTENT or W > UPSAMPLE_MAX_EXTENT:
        return f"H or W beyond {UPSAMPLE_MAX_EXTENT}"
    if N * H * W >= 2 ** 31:
        return "N * H * W reaches 2^31"
    if C > UPSAMPLE_MAX_CLASSES:
        return f"more than {UPSAMPLE_MAX_CLASSES} classes"
    if not 0.0 <= smoothing < 1.0:
        return f"label_smoothing {smoothing} outside [0, 1)"
    if has_weight and smoothing != 0.0:
        return "class weights together with label smoothing"
    return None


def upsampled_xent(x, y, align_corners=False, ignore_index=-100, weight=None, smoothing=0.0, grad_scale=1.0):
    """CE(up(x), y) for x [N, C, h, w] and class-index y [N, H, W]: (loss, gx [N, C, h, w] fp32 = grad_scale * dloss/dx),
    without a full-resolution [N, C, H, W] tensor.  A layout whose planes are not dense takes one .contiguous() of x."""
    require_gpu(x, "upsampled_xent")
    why = upsampled_xent_refusal(tuple(x.shape), x.dtype, tuple(y.shape), y.dtype, weight is not None, float(smoothing))
    if why is not None:
        raise NBDTHipError(f"upsampled_xent: {why}")
    if not _dense_planes(tuple(x.shape), tuple(x.stride())):
        x = x.contiguous()
    y = y.to(device=x.device, dtype=torch.int64).contiguous()
    if weight is not None:
        if weight.dim() != 1 or weight.shape[0] != x.shape[1]:
            raise NBDTHipError(f"upsampled_xent: {tuple(weight.shape)} class weights for {x.shape[1]} classes")
        weight = weight.detach().to(device=x.device, dtype=torch.float32).contiguous()
    N, C, h, w = x.shape
    H, W = y.shape[1:]
    _, hw, xi, xc = _seg_geom(x)
    ws = torch.empty((int(lib().nbdt_upsampled_xent_workspace_floats(N, H, W)),), dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    gx = torch.empty((N, C, h, w), dtype=torch.float32, device=x.device)
    check(lib().nbdt_upsampled_xent(ptr(x), ztype_of(x), N, C, h, w, xi, xc, ptr(y), H, W, int(bool(align_corners)),
                                    int(ignore_index), ptr(weight), float(smoothing), float(grad_scale), ptr(ws),
                                    ptr(loss), ptr(gx), stream_of(x)))
    return loss, gx
