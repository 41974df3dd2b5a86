"""ctypes binding of libwitw_hip.so — the C-ABI boundary declared in include/witw_hip.h.

There is no CPU fallback: if the library is missing it is built (hipcc) and if that fails, or a
call returns an error code, an exception is raised.
"""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_longlong, c_void_p

from . import build as _build

_LIB = None
_GUARDS = None

# name -> (restype, argtypes); mirrors include/witw_hip.h one-to-one
SIGNATURES = {
    'witw_last_error': (c_char_p, []),
    'witw_version': (c_int, []),
    'witw_last_kernel_variant': (c_char_p, []),
    'witw_last_conv_form': (c_char_p, []),
    'witw_device_check': (c_int, [c_int]),
    'witw_conv3x3_tile_n': (c_int, [c_int]),
    'witw_conv3x3_workgroup_waves': (c_int, [c_int] * 5),
    'witw_conv3x3_packed_floats': (c_longlong, [c_int, c_int]),
    'witw_conv3x3_bias_floats': (c_int, [c_int]),
    'witw_conv3x3_pack_weights': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_nchw_to_nhwc8': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'witw_conv3x3_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 10 + [c_void_p]),
    'witw_conv3x3_fwd_ex': (c_int, [c_void_p] * 9 + [c_int] * 8 + [c_float] + [c_int] * 3 + [c_void_p]),
    'witw_conv3x3_dil_skip': (c_int, [c_int]),
    'witw_conv3x3_packed_floats_wino': (c_longlong, [c_int, c_int]),
    'witw_conv3x3_pack_weights_wino': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'witw_conv3x3_fwd_wino': (c_int, [c_void_p] * 10 + [c_int] * 8 + [c_float] + [c_int] * 3 + [c_void_p]),
    'witw_conv3x3_wino': (c_int, [c_int]),
    'witw_conv3x3_wino_run': (c_int, [c_int]),
    'witw_conv3x3_wino_dma': (c_int, [c_int]),
    'witw_maxpool2x2_bwd': (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
    'witw_conv3x3_packed_floats_taps4': (c_longlong, [c_int, c_int]),
    'witw_conv3x3_pack_weights_taps4': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_conv3x3_fwd_taps4': (c_int, [c_void_p] * 7 + [c_int] * 6 + [c_float, c_int, c_void_p]),
    'witw_conv3x3_taps4_ksplit': (c_int, [c_int] * 5),
    'witw_conv3x3_fwd_taps4_ex': (c_int, [c_void_p] * 7 + [c_int] * 6 + [c_float] + [c_int] * 5 + [c_void_p]),
    'witw_conv3x3_wgrad_taps4': (c_int, [c_void_p] * 5 + [c_int] * 7 + [c_void_p]),
    'witw_nchw_to_nhwc': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'witw_conv3x3_wgrad_splits': (c_int, [c_int] * 5),
    'witw_conv3x3_wgrad_workspace_floats': (c_longlong, [c_int] * 6),
    'witw_conv3x3_wgrad': (c_int, [c_void_p] * 5 + [c_int] * 9 + [c_void_p]),
    'witw_adam_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_float, c_float, c_float, c_float, c_int,
                               c_void_p]),
    'witw_adam_step_multi': (c_int, [c_void_p] * 6 + [c_int, c_float, c_float, c_float, c_float, c_void_p]),
    'witw_conv3x3_first_pack': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'witw_conv3x3_first_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    'witw_conv3x3_bf16_mfma16': (c_int, [c_int]),
    'witw_conv3x3_bf16_wres': (c_int, [c_int]),
    'witw_conv3x3_bf16_packed_elems': (c_longlong, [c_int, c_int]),
    'witw_conv3x3_bf16_pack_weights': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'witw_conv3x3_bf16_pack_weights_ex': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_conv3x3_bf16_pack_weights_multi': (c_int, [c_void_p] * 7 + [c_int, c_void_p]),
    'witw_nchw_f32_to_nhwc_bf16': (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    'witw_conv3x3_bf16_fwd': (c_int, [c_void_p] * 4 + [c_int] * 10 + [c_void_p]),
    'witw_conv3x3_bf16_fwd_ex': (c_int, [c_void_p] * 7 + [c_int] * 11 + [c_void_p]),
    'witw_maxpool2x2_bwd_bf16': (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p]),
    'witw_octet_elems': (c_longlong, [c_int] * 4),
    'witw_nhwc_bf16_to_octet': (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    'witw_conv3x3_wgrad_bf16_workspace_floats': (c_longlong, [c_int] * 6),
    'witw_conv3x3_wgrad_bf16': (c_int, [c_void_p] * 5 + [c_int] * 9 + [c_void_p]),
    'witw_conv3x3_wgrad_bf16_nhwc_workspace_floats': (c_longlong, [c_int] * 6),
    'witw_conv3x3_wgrad_bf16_mfma16': (c_int, [c_int]),
    'witw_conv3x3_wgrad_bf16_nhwc': (c_int, [c_void_p] * 5 + [c_int] * 9 + [c_void_p]),
    'witw_conv3x3_f16x3_packed_elems': (c_longlong, [c_int, c_int]),
    'witw_conv3x3_f16x3_pack_weights': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'witw_nchw_f32_to_split_f16': (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    'witw_split_f16_to_f32': (c_int, [c_void_p, c_void_p, c_longlong, c_int, c_void_p]),
    'witw_conv3x3_f16x3_fwd': (c_int, [c_void_p] * 4 + [c_int] * 10 + [c_void_p]),
    'witw_conv3x3_f16x3_pack_weights_ex': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_conv3x3_f16x3_fwd_ex': (c_int, [c_void_p] * 8 + [c_int] * 11 + [c_void_p]),
    'witw_maxpool2x2_bwd_split': (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p]),
    'witw_octet_split_elems': (c_longlong, [c_int] * 4),
    'witw_split_f16_to_octet': (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    'witw_conv3x3_wgrad_f16x3_workspace_floats': (c_longlong, [c_int] * 6),
    'witw_conv3x3_wgrad_f16x3': (c_int, [c_void_p] * 6 + [c_int] * 9 + [c_void_p]),
    'witw_conv4x4s2_first_fwd': (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_float, c_void_p]),
    'witw_conv4x4s2_first_fwd_bf16': (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_float, c_void_p]),
    'witw_conv3x3_bf16_packed_elems_taps4': (c_longlong, [c_int, c_int]),
    'witw_conv3x3_bf16_pack_weights_taps4': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'witw_conv3x3_bf16_fwd_taps4': (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_float] + [c_int] * 3 + [c_void_p]),
    'witw_conv3x3_bf16_taps4_ksplit': (c_int, [c_int] * 5),
    'witw_conv3x3_bf16_fwd_taps4_splitk': (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p]),
    'witw_space_to_depth2_mosaic_bf16': (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    'witw_conv3x3_bf16_pack_weights_taps4_ex': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_conv3x3_bf16_fwd_taps4_plain': (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_float] + [c_int] * 3 + [c_void_p]),
    'witw_space_to_depth2_bf16': (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p] * 3),
    'witw_f32_to_bf16': (c_int, [c_void_p, c_void_p, c_longlong, c_void_p]),
    'witw_conv3x3_wgrad_bf16_taps4_workspace_floats': (c_longlong, [c_int] * 5),
    'witw_conv3x3_wgrad_bf16_taps4': (c_int, [c_void_p] * 5 + [c_int] * 7 + [c_void_p]),
    'witw_space_to_depth2': (c_int, [c_void_p, c_void_p] + [c_int] * 9 + [c_void_p, c_void_p, c_void_p]),
    'witw_space_to_depth2_mosaic': (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    'witw_taps4_splitk_finish': (c_int, [c_void_p, c_int, c_void_p, c_int, c_float] + [c_void_p] * 3 + [c_int] * 7 + [c_void_p]),
    'witw_gem_pool': (c_int, [c_void_p, c_void_p] + [c_int] * 8 + [c_float, c_void_p, c_void_p, c_void_p]),
    'witw_bn_workspace_floats': (c_longlong, [c_int] * 4),
    'witw_bn_train_stats': (c_int, [c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_float, c_float] + [c_void_p] * 8),
    'witw_bn_lrelu_bwd': (c_int, [c_void_p] * 8 + [c_int] * 6 + [c_float, c_void_p, c_void_p]),
    'witw_bn_lrelu_bwd_ex': (c_int, [c_void_p] * 8 + [c_int] * 6 + [c_float, c_int, c_void_p, c_void_p]),
    'witw_bn_partial_stats': (c_int, [c_void_p] + [c_int] * 6 + [c_void_p] * 4),
    'witw_bn_finalize_stats': (c_int, [c_void_p, c_void_p, c_longlong, c_void_p, c_void_p, c_float, c_float] + [c_void_p] * 6 + [c_int, c_void_p]),
    'witw_bn_lrelu_bwd_partial': (c_int, [c_void_p] * 4 + [c_int] * 7 + [c_void_p] * 3),
    'witw_bn_lrelu_bwd_apply': (c_int, [c_void_p] * 7 + [c_longlong] + [c_int] * 6 + [c_float, c_int, c_void_p]),
    'witw_depth_to_space2': (c_int, [c_void_p] * 3 + [c_int] * 7 + [c_void_p]),
    'witw_gem_pool_bwd': (c_int, [c_void_p] * 6 + [c_int] * 8 + [c_float, c_int, c_void_p]),
    'witw_embed_normalize_bwd': (c_int, [c_void_p] * 3 + [c_int, c_int, c_void_p]),
    'witw_exhaustive_triplet_loss_bwd': (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_float, c_float, c_void_p, c_void_p]),
    'witw_exhaustive_loss_slab_fwd': (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_float, c_float] + [c_void_p] * 3),
    'witw_exhaustive_loss_slab_sig': (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_float, c_float] + [c_void_p] * 3),
    'witw_exhaustive_loss_slab_bwd': (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_float, c_float, c_void_p]),
    'witw_sqdist_rect_bwd': (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p]),
    'witw_baseline_hard_slab_loss': (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_float, c_float, c_void_p, c_void_p]),
    'witw_baseline_hard_pairs': (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_float, c_float] + [c_void_p] * 4),
    'witw_sqdist_pairs_bwd_workspace_bytes': (c_longlong, [c_int] * 3),
    'witw_sqdist_pairs_bwd': (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 2 + [c_int] * 3 + [c_void_p] * 2),
    'witw_embed_normalize': (c_int, [c_void_p, c_int, c_int, c_void_p]),
    'witw_pairwise_sqdist': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'witw_row_sqnorm': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'witw_sqdist_gemm': (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p]),
    'witw_sqdist_pairs': (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p]),
    'witw_exhaustive_triplet_loss': (c_int, [c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    'witw_match_bwd_scratch_floats': (c_longlong, [c_int, c_int, c_int]),
    'witw_match_bwd': (c_int, [c_void_p] * 9 + [c_int] * 3 + [c_void_p]),
    'witw_match_workspace_floats': (c_longlong, [c_int, c_int]),
    'witw_match_fwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'witw_match_fwd_masked': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 6),
    'witw_match_fixed_workspace_floats': (c_longlong, [c_int, c_int]),
    'witw_match_fwd_fixed': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 6),
    'witw_match_spectrum_floats': (c_longlong, [c_longlong]),
    'witw_match_spectrum': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_match_dft_workspace_floats': (c_longlong, [c_int, c_int]),
    'witw_match_fwd_dft': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    'witw_match_fwd_dft_gap': (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 6),
    'witw_crop_overhead': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_l2_distance': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_rank_count': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_topk_smallest': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_longlong, c_void_p]),
    'witw_topk_workspace_bytes': (c_longlong, [c_int, c_int, c_int]),
    'witw_topk_smallest_ws': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_longlong, c_void_p, c_void_p]),
    'witw_topk_smallest_after': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_longlong, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    'witw_rank_count_thresh': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'witw_match_pairs': (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 4),
    'witw_match_pairs_impl': (c_int, [c_int]),
    'witw_match_profile': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 4),
    'witw_match_pairs_profile': (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 3),
    'witw_profile_hypotheses': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'witw_match_fwd_dft_masked': (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 7),
    'witw_match_pairs_masked': (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 5),
    'witw_match_pairs_count_masked': (c_int, [c_void_p] * 7 + [c_int] * 4 + [c_void_p] * 4),
    'witw_match_pairs_count': (c_int, [c_void_p] * 7 + [c_int] * 4 + [c_void_p] * 3),
    'witw_rank_count_band': (c_int, [c_void_p, c_void_p, c_float] + [c_void_p] * 4 + [c_int] * 3 + [c_void_p]),
    'witw_dropout2d_scales': (c_int, [c_void_p, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, c_void_p, c_int, c_int, c_int,
                                      c_float, c_void_p]),
    'witw_conv_first2_bf16_fwd': (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_void_p]),
    'witw_conv_first2_bf16_fwd_train': (c_int, [c_void_p] * 8 + [c_int] * 5 + [c_void_p]),
    'witw_conv3x3_bf16_gatebits_ok': (c_int, [c_int] * 5),
    'witw_conv3x3_bf16_fwd_gatebits': (c_int, [c_void_p] * 5 + [c_int] * 7 + [c_void_p]),
    'witw_triplet_loss_fwd': (c_int, [c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    'witw_triplet_loss_slab_fwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    'witw_triplet_loss_slab_sig': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    'witw_triplet_loss_slab_bwd': (c_int, [c_void_p] * 6 + [c_int, c_int, c_int, c_float, c_void_p]),
    'witw_triplet_loss_bwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p]),
    'witw_batch_hard_workspace_bytes': (c_longlong, [c_int, c_int]),
    'witw_batch_hard_fwd': (c_int, [c_void_p, c_int, c_float] + [c_void_p] * 7),
    'witw_batch_hard_slab_mine': (c_int, [c_void_p, c_int, c_int, c_int] + [c_void_p] * 6),
    'witw_batch_hard_merge_rows': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'witw_batch_hard_slab_loss': (c_int, [c_void_p] * 3 + [c_int] * 3 + [c_float, c_void_p, c_void_p]),
    'witw_batch_hard_pairs': (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_float] + [c_void_p] * 4),
    'witw_batch_hard_bwd': (c_int, [c_void_p] * 7 + [c_int, c_float, c_void_p]),
    'witw_match_bwd_pairs_scratch_bytes': (c_longlong, [c_int] * 3),
    'witw_match_bwd_pairs': (c_int, [c_void_p] * 8 + [c_int] * 4 + [c_void_p] * 4),
    'witw_resize_bilinear_normalize': (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_int, c_void_p]),
    'witw_resize_bilinear_normalize_batched': (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, c_void_p, c_int, c_void_p]),
    'witw_normalize': (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p, c_int, c_void_p]),
    'witw_polar_transform': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    'witw_polar_from_raw': (c_int, [c_void_p, c_void_p, c_int, c_void_p] + [c_int] * 7 + [c_void_p] * 3 + [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    'witw_bilinear_gather': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_longlong, c_longlong, c_void_p]),
    'witw_conv4x4_to_k3': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_k3_to_conv4x4': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'witw_jpeg_idct': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_void_p]),
    'witw_jpeg_to_rgb': (c_int, [c_void_p, c_void_p, c_int, c_longlong, c_void_p, c_void_p]),
    'witw_jpeg_huffman': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'witw_jpeg_huffman_selfsync': (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    'witw_jpeg_huffman_selfsync_threads': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'witw_jpeg_progressive_stage': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'witw_rotate_nearest': (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    'witw_baseline_rotate_batched': (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    'witw_baseline_roll_rows_batched': (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p]),
}


class WitwError(RuntimeError):
    pass


def lib_path():
    return _build.LIB


def load():
    """Load (building first if the .so is absent or stale) and type every entry point."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch ships its own libamdhip64.so (same SONAME as /opt/rocm's). It must be mapped BEFORE this
    # library so that both share ONE HIP runtime (streams and device pointers are exchanged); a
    # second runtime in the process fails with "no ROCm-capable device is detected".
    import torch  # noqa: F401
    path = os.environ.get('WITW_LIB') or _build.LIB      # WITW_LIB: an alternative build of the same ABI (A/B timing)
    if path == _build.LIB and (not os.path.exists(path) or (os.path.isdir(_build.CSRC) and _build.stale() and os.path.exists(_build.HIPCC))):
        _build.build(verbose=False)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    # hand-scheduled kernels are used only with a register allocation the parity tests have seen (build.py); decided HERE, after the
    # build, never at import time
    global _GUARDS
    _GUARDS = {}
    for name, (marker, force) in _build.guard_markers().items():
        tripped = path == _build.LIB and os.path.exists(marker) and force not in os.environ
        _GUARDS[name] = {'hand_scheduled_kernel': not tripped, 'forced': force in os.environ,
                         'detail': open(marker).read().strip().replace('\n', '; ') if tripped else ''}
        if tripped:
            import warnings
            warnings.warn('libwitw_hip: guard %r tripped -- a hand-scheduled kernel was compiled with an unvalidated register allocation '
                          '(%s); its compiler-scheduled replacement runs instead. Re-run the bf16 parity tests with %s=1 and update the '
                          'table in witw_amd/build.py.' % (name, _GUARDS[name]['detail'], force))
    if not _GUARDS['s16']['hand_scheduled_kernel']:
        lib.witw_conv3x3_bf16_mfma16(0)
    if not _GUARDS['wres']['hand_scheduled_kernel']:
        lib.witw_conv3x3_bf16_wres(0)
    return lib


def guards():
    """The register-allocation guards of build.py as this process sees them: name -> {'hand_scheduled_kernel': in use?, 'forced',
    'detail'}. 's16' / 'wres' act inside the library (switches set by load()); 'first2' is read by FOV_DSM._run (bf16)."""
    load()
    return _GUARDS


def check(rc, what):
    if rc != 0:
        msg = load().witw_last_error()
        raise WitwError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else ''))
