"""ctypes binding of the C ABI in include/qsae.h (libqsae_hip.so).

This is the only way the package reaches the GPU kernels; there is no CPU or eager-PyTorch
fallback.  If the library is missing or fails to load, every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional

_PKG = Path(__file__).resolve().parent
import os

# QSAE_HIP_LIB: another build of the same library (same-box A/B timing of two builds); default: the in-tree one
LIB_PATH = Path(os.environ["QSAE_HIP_LIB"]) if os.environ.get("QSAE_HIP_LIB") else _PKG / "lib" / "libqsae_hip.so"
# The debug build (same sources + -DQSAE_DEBUG_BUILD): process-wide qsae_debug_* switches and ablation kernels.  Never
# loaded by the package itself; tools/ and a few tests ask for it explicitly (use_library("debug")).
DEBUG_LIB_PATH = _PKG / "lib" / "libqsae_hip_debug.so"
ABI_VERSION = 4

OK = 0
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_WORKSPACE = -1, -2, -3, -4
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2

_vp, _i, _i64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

# name -> (restype, argtypes); must list every symbol declared in include/qsae.h
SIGNATURES = {
    "qsae_abi_version": (_i, []),
    "qsae_last_error": (C.c_char_p, []),
    "qsae_device_info": (_i, [C.POINTER(_i), C.c_char_p, _i]),
    "qsae_profile_sweep_events": (_i, [_vp, _vp]),
    "qsae_profile_event_create": (_i, [C.POINTER(_vp)]),
    "qsae_profile_event_destroy": (_i, [_vp]),
    "qsae_profile_event_elapsed_ms": (_i, [_vp, _vp, C.POINTER(_f)]),
    "qsae_profile_sweep_flop_fraction": (C.c_double, [_i]),
    "qsae_kperm_rows": (_i, [_vp, _i, _i, _vp, _vp]),
    "qsae_encode_dense": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp]),
    "qsae_encode_dense_kperm": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp]),
    "qsae_emu_w_bytes": (_sz, [_i, _i]),
    "qsae_emu_pack_w": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "qsae_encode_dense_emu_workspace_bytes": (_sz, [_i, _i]),
    "qsae_encode_dense_emu": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i64, _vp, _sz, _vp]),
    "qsae_encode_bits": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp]),
    "qsae_topk_rows": (_i, [_vp, _i64, _i, _i, _i, _vp, _vp, _i, _vp]),
    "qsae_encode_topk_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsae_encode_topk": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_encode_topk_kperm": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_encode_topk_latent": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _i, _vp, _sz, _vp]),
    "qsae_prefilter_w_bytes": (_sz, [_i, _i]),
    "qsae_prefilter_pack_w": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "qsae_encode_topk_prefilter_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsae_encode_topk_prefilter": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp, _sz, _i,
                                         C.POINTER(_i), _vp]),
    "qsae_binary_forward_prefilter": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _i64, _vp,
                                            _vp, _sz, _i, C.POINTER(_i), _vp]),
    "qsae_prefilter_submit": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _i64, _vp,
                                    _vp, _sz, _vp, _vp]),
    "qsae_prefilter_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _i64, _vp,
                                    _vp, _sz, _i, _vp]),
    "qsae_table_forward_prefilter": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _i64, _vp,
                                           _vp, _sz, _i, C.POINTER(_i), _vp]),
    "qsae_prefilter_submit_table": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _i64, _vp,
                                          _vp, _sz, _vp, _vp]),
    "qsae_prefilter_finish_table": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _i64, _vp,
                                          _vp, _sz, _i, _vp]),
    "qsae_densify": (_i, [_vp, _vp, _i, _i, _i, _vp, _i64, _vp]),
    "qsae_binary_row_bytes": (_i, [_i, _i]),
    "qsae_pack_binary": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "qsae_unpack_binary": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "qsae_decode_binary_sparse": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "qsae_decode_table_sparse": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "qsae_binary_soft_table": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "qsae_pack_ternary": (_i, [_vp, _i, _i, _vp, _vp]),
    "qsae_decode_ternary_dense": (_i, [_vp, _i64, _i, _i, _vp, _i, _vp, _vp]),
    "qsae_matryoshka_sizes": (_i, [_i, _i, _vp]),
    "qsae_pack_matryoshka": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "qsae_decode_matryoshka": (_i, [_vp, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "qsae_encode_bits_prefilter_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_encode_bits_prefilter": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _sz, C.POINTER(_i), _vp]),
    "qsae_encode_bits_prefilter_submit": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _sz, _vp, _vp]),
    "qsae_encode_bits_prefilter_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _sz, _i, _vp]),
    "qsae_encode_bits_band_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_encode_bits_band": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _sz, C.POINTER(_i), _vp]),
    "qsae_encode_bits_band_submit": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _sz, _vp, _vp]),
    "qsae_encode_bits_band_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i64, _vp, _sz, _i, _vp]),
    "qsae_pack_matryoshka_rows": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "qsae_decode_matryoshka_sparse": (_i, [_vp, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "qsae_split_dec_supported": (_i, [_i, _i, _i]),
    "qsae_expand_codes_bf16_bytes": (_sz, [_i, _i]),
    "qsae_expand_codes_bf16": (_i, [_vp, _i, _i, _vp, _vp]),
    "qsae_decode_ternary_dense_split": (_i, [_vp, _i64, _i, _i, _vp, _i, _vp, _vp]),
    "qsae_split_scale_bf16": (_i, [_vp, _i, _vp, _vp]),
    "qsae_decode_matryoshka_split": (_i, [_vp, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "qsae_pack_bits_gt": (_i, [_vp, _i64, _i, _i, _f, _vp, _i64, _vp]),
    "qsae_residual_update": (_i, [_vp, _vp, _sz, _f, _vp, _vp]),
    "qsae_threshold_ge": (_i, [_vp, _sz, _f, _vp, _vp]),
    "qsae_scale_bias_rows": (_i, [_vp, _i, _i, _f, _vp, _vp, _vp]),
    "qsae_sq_err_sum": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "qsae_activation_counts": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "qsae_activation_counts_bits": (_i, [_vp, _i64, _i, _i, _vp, _vp]),
    "qsae_coactivation_sparse": (_i, [_vp, _vp, _i, _i, _i, _vp, _i64, _vp]),
    "qsae_coactivation_bits_workspace_bytes": (_sz, [_i, _i]),
    "qsae_coactivation_bits": (_i, [_vp, _i64, _i, _i, _vp, _i, _vp, _i64, _vp, _sz, _vp]),
    "qsae_coactivation_partners_bits": (_i, [_vp, _i64, _i, _i, _vp, _vp, _i64, _vp, _sz, _vp]),
    "qsae_coactivation_partners_sparse": (_i, [_vp, _vp, _i, _i, _i, _vp, _i64, _vp]),
    "qsae_coactivation_partner_counts": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp]),
    "qsae_coactivation_partner_counts_dense": (_i, [_vp, _i64, _i, _i, _i64, _vp, _vp]),
    "qsae_token_lists_workspace_bytes": (_sz, [_i, _i]),
    "qsae_token_lists_count": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "qsae_token_lists_count_bits": (_i, [_vp, _i64, _i, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "qsae_token_lists_fill": (_i, [_vp, _sz, _vp, _vp, _i, _i, _vp, _i64, _vp]),
    "qsae_token_lists_regroup": (_i, [_vp, _i, _i, _vp, _i64, _vp, _vp, _vp]),
    "qsae_token_overlap_hist_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_token_overlap_hist": (_i, [_vp, _i64, _vp, _i, _vp, _i64, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "qsae_quantize_bits": (_i, [_vp, _i64, _i, _i, _i, _f, _i, _vp, _vp]),
    "qsae_atom_inv_norms": (_i, [_vp, _i64, _i, _i, _vp, _vp]),
    "qsae_cosine_compare_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_cosine_compare": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                 _vp, _sz, _vp]),
    "qsae_nearest_atoms_i8_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsae_nearest_atoms_i8": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_nearest_atoms_f32_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsae_nearest_atoms_f32": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "qsae_kmeans_assign_f32_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_kmeans_assign_f32": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "qsae_kmeans_update_f32_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_kmeans_update_f32": (_i, [_vp, _i64, _i, _i, _vp, _i, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "qsae_top_examples_compact_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_top_examples_compact": (_i, [_vp, _vp, _i, _i, _i, _i, _f, C.c_uint32, _vp, _vp, _sz, _vp]),
    "qsae_top_examples_dense_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_top_examples_dense": (_i, [_vp, _i64, _i, _i, _i, _f, C.c_uint32, _vp, _vp, _sz, _vp]),
    "qsae_top_examples_decode": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "qsae_quantization_error_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_quantization_error": (_i, [_vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "qsae_dataset_moments_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsae_dataset_moments_add": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_binary_soft_table_polarize_workspace_bytes": (_sz, [_i, _i]),
    "qsae_binary_soft_table_polarize": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_train_csr_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_train_csr": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_train_row_grad": (_i, [_vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "qsae_train_unit_grad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsae_train_unit_grad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _sz,
                                  _vp]),
    "qsae_train_col_sum_workspace_bytes": (_sz, [_i, _i]),
    "qsae_train_col_sum": (_i, [_vp, _i, _i, _vp, _vp, _sz, _vp]),
    "qsae_train_table_unit_grad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsae_train_table_unit_grad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _i64, _vp, _sz, _vp]),
    "qsae_transpose_rows": (_i, [_vp, _i, _i, _vp, _vp]),
    "qsae_train_pre_bits": (_i, [_vp, _i64, _i, _i, _vp, _i64, _vp]),
    "qsae_train_matryoshka_sign_rows": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "qsae_train_matryoshka_dpre": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp]),
    "qsae_train_gemm_tn": (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _vp, _i64, _vp]),
    "qsae_train_matryoshka_dsum_dense": (_i, [_vp, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "qsae_train_bits_csr_workspace_bytes": (_sz, [_i, _i]),
    "qsae_train_bits_csr": (_i, [_vp, _i64, _i, _i, _vp, _vp, _i64, _vp, _sz, _vp]),
    "qsae_train_matryoshka_dsum_lists_workspace_bytes": (_sz, [_i, _i64, _i, _i]),
    "qsae_train_matryoshka_dsum_lists": (_i, [_vp, _vp, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_train_matryoshka_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "qsae_train_matryoshka_secant": (_i, [_vp, _f, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "qsae_normalize_columns_table": (_i, [_vp, _i, _i, _vp, _vp]),
    "qsae_train_ternary_rows": (_i, [_vp, _i, _i, _vp, _vp]),
    "qsae_train_ternary_dpre": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "qsae_train_ternary_dweight": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "qsae_blatent_binarize": (_i, [_vp, _i, _i, _f, _vp, _vp, _vp]),
    "qsae_train_blatent_dpre": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "qsae_train_blatent_dweight": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp]),
    "qsae_train_mask_workspace_bytes": (_sz, [_i, _i]),
    "qsae_train_mask_init": (_i, [_vp, _vp, _i, _i, _i64, _vp, _sz, _vp]),
    "qsae_train_mask_update": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i64, _vp, _sz, _vp]),
    "qsae_adam_step": (_i, [_vp, _vp, _vp, _vp, C.c_longlong, _f, _f, _f, _f, _f, _f, _vp]),
    "qsae_adam_step_prefilter": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _f, _f, _f, _vp, _vp, _vp]),
    "qsae_rows_nan_bitmap": (_i, [_vp, _i, _i64, _i, _vp, _vp]),
    "qsae_gather_rows": (_i, [_vp, _i, _i64, _i, _vp, _i, _vp, _vp, _vp]),
    "qsae_trainer_loss_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsae_trainer_loss": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_double, _vp, _vp, _vp, _sz, _vp]),
    "qsae_tensor_stats_workspace_bytes": (_sz, [_vp, _i]),
    "qsae_tensor_stats": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "qsae_activity_add_compact": (_i, [_vp, _vp, _i, _i, _i, _i64, _vp, _vp, _vp]),
    "qsae_activity_add_bits": (_i, [_vp, _i64, _i, _i, _vp, _i, _i64, _vp, _vp, _vp]),
    "qsae_activity_add_dense": (_i, [_vp, _i64, _i, _i, _i64, _vp, _vp, _vp]),
    "qsae_activity_summary_workspace_bytes": (_sz, [_i]),
    "qsae_activity_summary": (_i, [_vp, _vp, _vp, _i, _i64, _i64, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_resample_row_weights": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp, _vp]),
    "qsae_resample_draw_workspace_bytes": (_sz, [_i]),
    "qsae_resample_draw": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsae_resample_alive_stats": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "qsae_resample_write_table": (_i, [_vp, _vp, _i, _vp, _i64, _i, _i, _i, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _i64, _vp, _vp]),
    "qsae_resample_write_binary": (_i, [_vp, _vp, _i, _vp, _i64, _i, _i, _i, _i, _vp, _vp, C.c_double, _i, C.c_double, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
}

# name -> (restype, argtypes) of the qsaex_* entry points of include/qsae_ext.h (csrc/auxk.hip): the same library, bound next
# to SIGNATURES; they move into that table when qsae.h takes them in.  Must list every symbol declared in qsae_ext.h.
EXT_SIGNATURES = {
    "qsaex_encode_topk_units_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsaex_encode_topk_units": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "qsaex_auxk_loss_workspace_bytes": (_sz, [_i, _i]),
    "qsaex_auxk_loss": (_i, [_vp, _vp, _vp, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes) of the qsaec_* entry points of include/qsae_curve.h (csrc/sparsity_curve.hip): a table of its
# own for the same reason.  Must list every symbol declared in qsae_curve.h.
CURVE_SIGNATURES = {
    "qsaec_prefix_errors_binary_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsaec_prefix_errors_binary": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                        _sz, _vp]),
    "qsaec_prefix_errors_table_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsaec_prefix_errors_table": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz,
                                       _vp]),
}

# name -> (restype, argtypes) of the qsaen_* entry points of include/qsae_nested.h (csrc/nested.hip): the nested-dictionary
# objective of the top-k SAEs, a table of its own for the same reason.  Must list every symbol declared in qsae_nested.h.
NESTED_SIGNATURES = {
    "qsaen_decode_nested_binary": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _i, _vp, _vp]),
    "qsaen_decode_nested_table": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i, _vp, _vp]),
    "qsaen_row_grad_nested": (_i, [_vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "qsaen_train_unit_grad_nested_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsaen_train_unit_grad_nested": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp,
                                          _vp, _vp, _sz, _vp]),
    "qsaen_train_table_unit_grad_nested_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsaen_train_table_unit_grad_nested": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i64, _vp,
                                                _sz, _vp]),
}

# name -> (restype, argtypes) of the qsaeb_* entry points of include/qsae_batch.h (csrc/batch_topk.hip, batch_topk_decode.hip):
# BatchTopK -- the batch-wide selection, the threshold selection and the ragged row operations -- a table of its own for the
# same reason.  Must list every symbol declared in qsae_batch.h.
BATCH_SIGNATURES = {
    "qsaeb_batch_select_workspace_bytes": (_sz, [_i, _i]),
    "qsaeb_batch_select": (_i, [_vp, _i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _f, _vp, _sz, _vp]),
    "qsaeb_threshold_select_workspace_bytes": (_sz, [_i, _i]),
    "qsaeb_threshold_select": (_i, [_vp, _i, _i, _vp, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    "qsaeb_decode_ragged_binary": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    "qsaeb_decode_ragged_table": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "qsaeb_row_grad_ragged": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "qsaeb_csr_ragged_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsaeb_csr_ragged": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
}

# name -> (restype, argtypes) of the qsaem_* entry points of include/qsae_nested_batch.h (csrc/nested_ragged.hip): the nested
# levels over the ragged rows of BatchTopK, a table of its own for the same reason.  Must list every symbol declared in
# qsae_nested_batch.h.
NESTED_BATCH_SIGNATURES = {
    "qsaem_decode_nested_ragged_binary": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _i, _vp, _vp, _vp]),
    "qsaem_decode_nested_ragged_table": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i, _vp, _vp, _vp]),
    "qsaem_row_grad_nested_ragged": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
}

# name -> (restype, argtypes) of the qsaek_* entry points of include/qsae_multik.h (csrc/multi_topk.hip): the Multi-TopK
# objective of the top-k SAEs, a table of its own for the same reason.  Must list every symbol declared in qsae_multik.h.
MULTIK_SIGNATURES = {
    "qsaek_decode_multik_binary": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _vp, _vp, _i, _vp, _vp]),
    "qsaek_decode_multik_table": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i, _vp, _vp]),
    "qsaek_row_grad_multik": (_i, [_vp, _i, _i, _vp, _i, _i, _f, _vp, _vp, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "qsaek_train_unit_grad_multik_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsaek_train_unit_grad_multik": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _f, _vp, _vp, _vp,
                                          _vp, _vp, _sz, _vp]),
    "qsaek_train_table_unit_grad_multik_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsaek_train_table_unit_grad_multik": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i64, _vp,
                                                _sz, _vp]),
}

# name -> (restype, argtypes) of the qsaej_* entry points of include/qsae_jump.h (csrc/jumprelu.hip): JumpReLU -- the per-unit
# threshold selection and the thresholds' pseudo-gradient -- a table of its own for the same reason.  Must list every symbol
# declared in qsae_jump.h.
JUMP_SIGNATURES = {
    "qsaej_jump_select_workspace_bytes": (_sz, [_i, _i, _i]),
    "qsaej_jump_select": (_i, [_vp, _vp, _i, _i, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "qsaej_threshold_grad": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
}

# name -> (restype, argtypes) of the qsaed_* entry points of include/qsae_jump_dense.h (csrc/jump_dense.hip): the dense (uncapped)
# JumpReLU encoder -- the thresholds in the epilogue of the encoder's contraction -- a table of its own for the same reason.  Must
# list every symbol declared in qsae_jump_dense.h.
JUMP_DENSE_SIGNATURES = {
    "qsaed_encode_jump_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsaed_encode_jump": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                               _vp]),
}

# name -> (restype, argtypes) of the qsaebd_* entry points of include/qsae_batch_dense.h (csrc/batch_dense.hip): the dense
# BatchTopK encoder -- a scalar floor in the epilogue of the encoder's contraction, the batch-wide selection over the candidates
# and its certificate -- a table of its own for the same reason.  Must list every symbol declared in qsae_batch_dense.h.
BATCH_DENSE_SIGNATURES = {
    "qsaebd_encode_batch_topk_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "qsaebd_encode_batch_topk": (_i, [_vp, _i64, _vp, _i64, _vp, _i, _i, _i, _i, _i64, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _f, _vp, _sz, _vp]),
}

# name -> (restype, argtypes) of the qsaer_* entry points of include/qsae_recycle.h (csrc/prefilter_topk.hip): the
# forward-in-one-call prefilter entry points on a recycled dense latent -- their namesakes of SIGNATURES plus (stale_idx,
# stale_k) -- a table of its own for the same reason.  Must list every symbol declared in qsae_recycle.h.
RECYCLE_SIGNATURES = {
    "qsaer_" + name[len("qsae_"):]: (SIGNATURES[name][0], SIGNATURES[name][1] + [_vp, _i])
    for name in ("qsae_binary_forward_prefilter", "qsae_table_forward_prefilter", "qsae_prefilter_submit",
                 "qsae_prefilter_submit_table")
}

# name -> (restype, argtypes) of the qsaeo_* entry points of include/qsae_optim.h (csrc/optim_recipe.hip): the recipe around the
# Adam step -- the joint gradient norm and its clip coefficient, the steps that read it and carry the weights' moving average,
# the projection of the decoder gradient -- a table of its own for the same reason.  Must list every symbol declared in
# qsae_optim.h.
OPTIM_SIGNATURES = {
    "qsaeo_project_columns": (_i, [_vp, _vp, _i, _i, _i64, _vp]),
    "qsaeo_grad_norm_workspace_bytes": (_sz, [_vp, _i]),
    "qsaeo_grad_norm": (_i, [_vp, _vp, _i, C.c_double, _vp, _vp, _vp, _sz, _vp]),
    "qsaeo_adam_step": (_i, SIGNATURES["qsae_adam_step"][1][:-1] + [_vp, _vp, _f, _vp]),
    "qsaeo_adam_step_prefilter": (_i, SIGNATURES["qsae_adam_step_prefilter"][1][:-3] + [_vp, _vp, _vp, _f, _vp, _vp, _vp]),
}

# name -> (restype, argtypes) of the qsaew_* entry points of include/qsae_wide.h (csrc/wide.hip): per-row top-k over hidden
# slabs -- the plan, the S-way merge of the slabs' lists, and the two whole selections -- a table of its own for the same reason.
# Must list every symbol declared in qsae_wide.h.
WIDE_SIGNATURES = {
    "qsaew_slab_plan": (_i, [_i, _i, _i, C.POINTER(_i)]),
    "qsaew_merge_topk": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(_i), _vp, _vp, _vp, _i64, _vp]),
    "qsaew_encode_topk_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "qsaew_encode_topk": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp, _sz, _vp]),
    "qsaew_encode_topk_prefilter_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "qsaew_encode_topk_prefilter": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp, _sz, _i,
                                          C.POINTER(_i), _vp]),
}


class QsaeError(RuntimeError):
    """A libqsae_hip call returned a non-zero status."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libqsae_hip error {code}: {message}")
        self.code = code


_libs = {}          # "product" / "debug" -> CDLL
_active = "product"


def _open(path: Path) -> C.CDLL:
    if not path.exists():
        raise RuntimeError(
            f"{path} is missing: build it with `python -m quantizedsae_amd.build` "
            "(hipcc --offload-arch=gfx950).  quantizedsae_amd has no CPU / eager fallback.")
    lib = C.CDLL(str(path))
    for name, (res, args) in list(SIGNATURES.items()) + list(EXT_SIGNATURES.items()) + list(CURVE_SIGNATURES.items()) \
            + list(NESTED_SIGNATURES.items()) + list(BATCH_SIGNATURES.items()) + list(NESTED_BATCH_SIGNATURES.items()) + list(MULTIK_SIGNATURES.items()) \
            + list(JUMP_SIGNATURES.items()) + list(JUMP_DENSE_SIGNATURES.items()) \
            + list(BATCH_DENSE_SIGNATURES.items()) + list(RECYCLE_SIGNATURES.items()) + list(OPTIM_SIGNATURES.items()) \
            + list(WIDE_SIGNATURES.items()):
        fn = getattr(lib, name)   # AttributeError here means the library is stale
        fn.restype = res
        fn.argtypes = args
    if lib.qsae_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{path.name}: ABI version mismatch; rebuild it")
    return lib


def load() -> C.CDLL:
    """The library the package computes with: libqsae_hip.so (loaded once).  Raises RuntimeError if it is missing --
    no fallback.  Inside a `use_library("debug")` block (tests / tools only) it is the debug build instead."""
    lib = _libs.get(_active)
    if lib is None:
        lib = _libs[_active] = _open(LIB_PATH if _active == "product" else DEBUG_LIB_PATH)
    return lib


class use_library:
    """Context manager for tests and tools: route the package's calls to the debug build (qsae_debug_* switches,
    ablation kernels) for the duration of the block.  Not thread-safe, not for product code."""

    def __init__(self, which: str):
        if which not in ("product", "debug"):
            raise ValueError(which)
        self.which = which

    def __enter__(self):
        global _active
        self.prev, _active = _active, self.which
        return load()

    def __exit__(self, *exc):
        global _active
        _active = self.prev
        return False


def check(code: int) -> None:
    if code != OK:
        msg = load().qsae_last_error()
        raise QsaeError(code, msg.decode(errors="replace") if msg else "")
