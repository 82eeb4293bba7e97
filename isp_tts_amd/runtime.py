"""ctypes binding of libispk.so (the C ABI declared in include/ispk.h) and thin tensor-level wrappers.

PyTorch here is plumbing only: it owns device memory and the stream.  Every wrapper passes raw
`data_ptr()`s and the CURRENT torch stream to the library, so launches are ordered with torch ops and are
capturable in a HIP graph.  There is no CPU fallback anywhere: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch
from torch import Tensor

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libispk.so")

EP_GELU, EP_SILU, EP_MASK_ACC, EP_MASK_OUT, EP_BIAS_ROW, EP_MASK_COL, EP_OUT_BF16, EP_RESID_BF16, EP_ROWS_T, EP_OUT_SPLIT = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512)

_P, _I32, _I64, _U32, _F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float
_U64, _F64 = ctypes.c_uint64, ctypes.c_double

# name -> argtypes; must list EVERY symbol of include/ispk.h (tests/test_abi.py checks header == this table == .so)
SIGNATURES = {
    "ispk_abi_version": [],
    "ispk_last_error_string": [],
    "ispk_device_info": [ctypes.c_char_p, _I32],
    "ispk_mas_f32": [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I64, _I64, _P],
    "ispk_layernorm_f32": [_P, _I64, _P, _P, _P, _P, _I64, _I32, _P, _P, _I64, _I32, _I32, _F32, _P],
    "ispk_layernorm_f32_bf16": [_P, _I64, _P, _P, _P, _P, _I64, _I32, _P, _P, _I64, _I32, _I32, _F32, _P],
    "ispk_gemm_f32_tile": [_I32, _I32, _I32],
    "ispk_gemm_f32": [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _I32, _U32, _I32, _I64, _P],
    "ispk_gemm_f32_batched": [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I32, _I32, _I32, _I32, _P],
    "ispk_gemm_bf16_gelu_train": [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _F32, _U64, _P],
    "ispk_gemm_bf16_gelu_bwd": [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I32, _I32, _I32, _F32, _U64, _P],
    "ispk_segments_f32": [_P, _I32, _P],
    "ispk_stage_weights": [_P, _I32, _P],
    "ispk_fill_zero": [_P, _I64, _P],
    "ispk_scale_f32": [_P, _I64, _P, _F32, _P],
    "ispk_sum_scalars_f32": [_P, _P, _I32, _P, _P],
    "ispk_exp_pad_f32": [_P, _P, _I32, _I32, _P],
    "ispk_sqrt_scale_f32": [_P, _P, _I32, _F32, _P],
    "ispk_copy2d_f32": [_P, _I64, _P, _I64, _I32, _I32, _P],
    "ispk_permute021_f32": [_P, _P, _I32, _I32, _I32, _P],
    "ispk_conv_weight_flip_f32": [_P, _P, _I32, _I32, _I32, _P],
    "ispk_gemm_bf16_last_variant": [],
    "ispk_gemm_bf16": [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _I32, _U32, _I32, _I64, _P],
    "ispk_gemm_bf16_splitk_plan": [_I32, _I32, _I32, _U32],
    "ispk_gemm_bf16_splitk": [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _I32, _U32, _P, _I32, _P],
    "ispk_ffn_bf16": [_P, _I64, _P, _I64, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I32, _I32, _I32, _U32, _P],
    "ispk_ffn_pack_w2_bf16": [_P, _I64, _I32, _I32, _P, _P],
    "ispk_ffn_bf16_prenorm": [_P, _I64, _P, _P, _F32, _P, _I64, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _U32, _P, _F32, _P],
    "ispk_ffn_chunk_w2_bf16": [_P, _I64, _I32, _I32, _P, _P],
    "ispk_ffn_bf16_prenorm2_split": [_P, _I64, _P, _P, _F32, _P, _P, _P, _I64, _I32, _I32, _I32, _I32, _P],
    "ispk_ffn_combine_ln_f32": [_P, _I64, _P, _I64, _I32, _P, _P, _I64, _P, _P, _F32, _I32, _P, _I64, _I32, _I32, _I32, _P],
    "ispk_ffn_bf16_prenorm2": [_P, _I64, _P, _P, _F32, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _U32, _P, _F32, _P],
    "ispk_attn_out_ffn_bf16": [_P, _I64, _P, _I64, _P, _P, _P, _F32, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _U32, _P, _F32, _P],
    "ispk_attn_out_ffn_qkv_bf16": [_P, _I64, _P, _I64, _P, _P, _P, _F32, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _U32, _P, _P, _F32,
                                   _P, _P, _I64, _P],
    "ispk_chunk_k16_bf16": [_P, _I64, _I32, _I32, _P, _P],
    "ispk_attn_out_ffn_norm_bf16": [_P, _I64, _P, _I64, _P, _P, _P, _F32, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _U32, _P, _P, _F32,
                                    _I32, _P, _I64, _I32, _P],
    "ispk_attn_out_ffn_split_bf16": [_P, _I64, _P, _I64, _P, _P, _P, _F32, _P, _P, _P, _U32, _P, _I64, _I32, _I32, _I32, _I32, _P],
    "ispk_gemm_bf16_lnin": [_P, _I64, _P, _P, _P, _F32, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _I32, _U32, _P],
    "ispk_linear_small_f32": [_P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _I32, _I32, _I32, _U32, _P],
    "ispk_alibi_mqa_attn_f32": [_P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _I32, _I32, _I32, _P],
    "ispk_alibi_mqa_attn_bf16": [_P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _I32, _I32, _I32, _P],
    "ispk_alibi_mqa_attn_bf16_tiles": [_P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _I32, _I32, _I32, _I32, _P],
    "ispk_cast_f32_bf16": [_P, _I64, _P, _I64, _I32, _I32, _P],
    "ispk_split_f16": [_P, _I64, _P, _P, _I64, _I32, _I32, _P],
    "ispk_gemm_split_f16_tile": [_I32, _I32, _I32],
    "ispk_gemm_split_f16": [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _P, _P, _I64, _P, _I32, _I32, _I32, _U32, _I32,
                            _I64, _P],
    "ispk_layernorm_f32_split": [_P, _I64, _P, _P, _P, _P, _I64, _I32, _P, _P, _I64, _I64, _I32, _I32, _F32, _P],
    "ispk_alibi_mqa_attn_split_f16": [_P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _I64, _I32, _I32, _I32, _P],
    "ispk_flow_mix_f32": [_P, _P, _P, _F32, _P, _P, _I32, _I32, _I32, _P],
    "ispk_flow_finish_f32": [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P],
    "ispk_flow_head_f32": [_P, _I64, _P, _P, _F32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_flow_euler_f32": [_P, _P, _F32, _P, _P, _I32, _I32, _I32, _P],
    "ispk_infer_features_f32": [_P, _P, _P, _P, _P, _F32, _F32, _F32, _F32, _F32, _P, _P, _I32, _I32, _P],
    "ispk_infer_features_round_f32": [_P, _P, _P, _P, _P, _F32, _F32, _F32, _F32, _F32, _P, _P, _I32, _I32, _P],
    "ispk_hard_regulate_f32": [_P, _P, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P],
    "ispk_hard_regulate_bwd_f32": [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P],
    "ispk_hard_average_f32": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _P],
    "ispk_embed_tokens_f32": [_P, _P, _I64, _I32, _P, _P, _P, _I32, _I32, _I32, _P],
    "ispk_embed_tokens_qkv": [_P, _P, _I64, _I32, _P, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_add_speaker_f32": [_P, _P, _I64, _I32, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_add_speaker_out_f32": [_P, _P, _P, _I64, _I32, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_speaker_grad_f32": [_P, _P, _I32, _P, _P, _I64, _P, _I64, _I32, _I32, _I32, _I32, _I32, _P],
    "ispk_time_embedding_f32": [_P, _I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _P, _P],
    "ispk_length_regulate_f32": [_P, _P, _P, _P, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P],
    "ispk_length_regulate_split_bf16": [_P, _P, _P, _P, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P],
    "ispk_length_regulate_qkv_bf16": [_P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _F32, _P, _P, _I64, _I32, _I32, _I32, _I32, _I32,
                                      _I32, _P],
    "ispk_length_regulate_split_f16": [_P, _P, _P, _P, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P],
    "ispk_pad_rows_f32": [_P, _I64, _I64, _I64, _P, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_masked_instnorm_f32": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F32, _P],
    "ispk_aligner_scores_f32": [_P, _I64, _P, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_aligner_scores_fast_f32": [_P, _I64, _P, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_soft_average_f32": [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P],
    "ispk_transpose_f32": [_P, _I64, _P, _I64, _I32, _I32, _P],
    "ispk_gemm_tn_f32": [_P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _I32, _P, _I64, _P],
    "ispk_gemm_tn_bf16": [_P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _I32, _P, _I64, _P],
    "ispk_gemm_tn_b16": [_P, _I64, _P, _I64, _P, _I64, _I32, _I32, _I32, _P, _I32, _P, _I64, _P],
    "ispk_gelu_f32_bf16": [_P, _P, _I64, _F32, _U64, _P],
    "ispk_gelu_bf16": [_P, _P, _I64, _F32, _U64, _P],
    "ispk_gelu_bwd_b16": [_P, _P, _P, _I64, _F32, _U64, _P],
    "ispk_gelu_bwd_bf16": [_P, _P, _P, _I64, _F32, _U64, _P],
    "ispk_gemm_tn_last_plan": [_P, _P],
    "ispk_gemm_tn_batched_f32": [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I32, _I32, _I32, _I32, _P, _I32, _P, _I64, _P],
    "ispk_layernorm_bwd_f32": [_P, _I64, _P, _I64, _P, _P, _P, _I64, _I32, _P, _P, _P, _I64, _I64, _I32, _F32, _P],
    "ispk_layernorm_bwd_dual_f32": [_P, _I64, _P, _I64, _P, _P, _P, _I64, _I32, _P, _P, _P, _I64, _I64, _I32, _F32, _P, _I64, _P],
    "ispk_gelu_f32": [_P, _P, _I64, _F32, _U64, _P],
    "ispk_gelu_bwd_f32": [_P, _P, _P, _I64, _F32, _U64, _P],
    "ispk_dropout_mask_u8": [_P, _I64, _F32, _U64, _P],
    "ispk_alibi_mqa_attn_train_f32": [_P, _I64, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _F32, _U64, _P],
    "ispk_alibi_mqa_attn_bwd_f32": [_P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _P, _F32, _U64, _P],
    "ispk_alibi_mqa_attn_train_bf16": [_P, _I64, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _F32, _U64, _P],
    "ispk_alibi_mqa_attn_bwd_bf16": [_P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _F32, _U64, _P],
    "ispk_mel_loss_f32": [_P, _P, _P, _P, _P, _P, _F32, _I32, _I32, _I32, _P],
    "ispk_acoustic_metrics_f32": [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P, _I64, _I64, _P, _P, _I64, _P, _I32,
                                  _I32, _I32, _I32, _I32, _P],
    "ispk_dtw_f32": [_P, _I64, _I64, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _P],
    "ispk_mcd_dtw_f32": [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I32,
                         _I32, _I32, _I32, _I32, _P],
    "ispk_audio_features_f32": [_P, _I64, _P, _P, _I64, _P, _I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F32, _F32, _F32,
                                _F32, _P],
    "ispk_resample_f32": [_P, _I64, _I64, _P, _P, _I64, _P, _P, _I64, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P],
    "ispk_feature_stats_f64": [_P, _I64, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _P],
    "ispk_audio_measure_f64": [_P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _I32, _F64, _I32, _I32, _F64,
                               _F64, _P],
    "ispk_audio_apply_f32": [_P, _I64, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _P],
    "ispk_pcm16": [_P, _I64, _P, _P, _I64, _I32, _I32, _I32, _U64, _P],
    "ispk_aligner_scores_bwd_f32": [_P, _P, _P, _P, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _I32, _F32, _P],
    "ispk_masked_instnorm_bwd_f32": [_P, _P, _P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _F32, _P],
    "ispk_soft_average_bwd_f32": [_P, _P, _P, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_flow_loss_bwd_f32": [_P, _P, _P, _F32, _P, _I32, _I32, _I32, _P],
    "ispk_adaln_bwd_f32": [_P, _I64, _P, _I64, _P, _I64, _P, _P, _I64, _I32, _P, _P, _I64, _I32, _I32, _I32, _F32, _P],
    "ispk_time_embedding_bwd_f32": [_P, _I32, _P, _P, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _P],
    "ispk_attn_ctc_loss_f32": [_P, _P, _P, _F32, _P, _I64, _P, _P, _F32, _I32, _I32, _I32, _P],
    "ispk_attn_bin_loss_f32": [_P, _P, _F32, _P, _P, _P, _F32, _I32, _I32, _I32, _P],
    "ispk_mel_grad_rows_f32": [_P, _P, _P, _I32, _I32, _I32, _P],
    "ispk_colsum_f32": [_P, _I64, _I64, _I32, _P, _P, _I64, _P, _P],
    "ispk_smallk_wgrad_f32": [_P, _I64, _P, _I64, _I64, _I32, _I32, _P, _I64, _P, _P],
    "ispk_embedding_bwd_f32": [_P, _P, _I64, _I32, _I32, _I32, _P, _I64, _P],
    "ispk_grad_sqnorm_f32": [_P, _I64, _P, _P, _P],
    "ispk_adamw_f32": [_P, _P, _P, _P, _I64, _I64, _F32, _F32, _F32, _F32, _F32, _I32, _P, _F32, _F32, _P],
    "ispk_adamw_f32_dev": [_P, _P, _P, _P, _I64, _I64, _P, _P, _P],
    "ispk_adam_args_f32": [_F32, _F32, _F32, _F32, _F32, _I32, _F32, _F32, _P],
    "ispk_set_dropout_seed_source": [_P],
    "ispk_vocoder_unfold": [_P, _I32, _I64, _I64, _I64, _P, _P, _I32, _I64, _P, _I32, _I32, _I32, _I32, _P],
    "ispk_dwconv7_ln_f32": [_P, _I64, _P, _P, _P, _P, _F32, _P, _P, _I32, _I64, _I32, _I32, _I32, _P],
    "ispk_istft_head_f32": [_P, _I64, _P, _P, _I64, _P, _I64, _P, _I32, _I32, _I32, _P],
    "ispk_hifigan_tile_rows": [],
    "ispk_hifigan_conv_f32": [_P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _F32,
                              _I32, _P],
    "ispk_hifigan_conv_bf16": [_P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _F32,
                               _I32, _P],
    "ispk_hifigan_upsample_f32": [_P, _I64, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _P],
    "ispk_hifigan_upsample_bf16": [_P, _I64, _P, _P, _P, _I64, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _P],
    "ispk_hifigan_post_f32": [_P, _I64, _P, _P, _P, _I32, _P, _I64, _P, _I32, _I32, _I32, _I32, _F32, _P],
}

_lib = None


class IspkError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Loads libispk.so.  Fails loudly when it has not been built (`python -m isp_tts_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IspkError(f"{LIB_PATH} is missing: the HIP extension was not built "
                            f"(run `python -m isp_tts_amd.build` or `__graft_entry__.build()`); there is no CPU fallback")
        handle = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_char_p if name == "ispk_last_error_string" else ctypes.c_int32
        if handle.ispk_abi_version() != 2:
            raise IspkError(f"libispk.so ABI version {handle.ispk_abi_version()} != 2 (rebuild: python -m isp_tts_amd.build)")
        _lib = handle
    return _lib


class LaunchProfiler:
    """Optional per-launch timing with HIP events on the launch stream (used by bench.py for the roofline object).
    Each record: (kernel label, algorithmic FLOPs, algorithmic HBM bytes, start event, end event)."""

    def __init__(self):
        self.records = []

    def summary(self) -> dict:
        """label -> {launches, total_ms, avg_us, flops, bytes} (call after a device synchronise)."""
        out: dict = {}
        for label, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(label, {"launches": 0, "total_ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["total_ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        for d in out.values():
            d["avg_us"] = 1e3 * d["total_ms"] / d["launches"]
        return out


_profiler: Optional[LaunchProfiler] = None


def set_profiler(p: Optional[LaunchProfiler]) -> None:
    global _profiler
    _profiler = p


# epilogue instances launch_panel() in csrc/gemm.hip compiles: qkv (bf16 out), FFN1 (bf16 out + GELU), out-projection
# (mask-acc + residual), to_mel (ROWS_T + mask-out + bias)
_PANEL_EPS = (64, 65, 4 | (1 << 17), 256 | 8 | (1 << 16))


def _launch(label: str, flops: float, nbytes: float, fn, *args) -> None:
    if _profiler is None:
        _check(fn(*args), label)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn(*args)
    e1.record()
    _check(rc, label)
    if label == "gemm_bf16_kernel":   # resolve to the instance the library actually dispatched
        v = lib().ispk_gemm_bf16_last_variant()
        if v // 1000 == 1:   # panel kernel <KC, EP>: EP = the compile-time epilogue instance (-1: the generic one)
            ep = (args[13] & 0xffff) | ((1 << 16) if args[6] else 0) | ((1 << 17) if args[7] else 0)
            label = f"gemm_bf16_panel_kernel<{v % 1000},{ep if ep in _PANEL_EPS else -1}>"
        else:
            label = {2: f"gemm_bf16_wide_kernel<{(v % 1000) // 10},{v % 10}>",
                     3: f"gemm_bf16_kernel<{(v % 1000) // 10},{v % 10}>"}.get(v // 1000, label)
    elif label.startswith("gemm_tn_b16_kernel") and lib().ispk_gemm_tn_last_plan(None, None) == 4:
        label = "gemm_tn_dma_kernel" + label[len("gemm_tn_b16_kernel"):]      # the LDS-DMA kernel, not the register-staged one
    _profiler.records.append((label, flops, nbytes, e0, e1))


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().ispk_last_error_string()
        raise IspkError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def _dev(*tensors: Optional[Tensor]) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise IspkError("isp_tts_amd kernels need GPU tensors (got a CPU tensor); there is no CPU fallback")


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def device_info() -> tuple[str, int]:
    buf = ctypes.create_string_buffer(256)
    n = lib().ispk_device_info(buf, 256)
    if n <= 0:
        _check(n if n != 0 else -1, "ispk_device_info")
    return buf.value.decode(), n


def _rows2d(t: Tensor) -> Tensor:
    """[..., D] -> [rows, D] view with unit inner stride (copies only when the layout requires it)."""
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t.reshape(-1, t.shape[-1])


# ------------------------------------------------------------------------------------------------- MAS
def mas(logits: Tensor, text_len: Tensor, mel_len: Tensor, want_dur: bool = True, want_path: bool = False):
    """ispk_mas_f32.  logits fp32 [B,M,L] (unit stride on L), lengths int64 [B] on the same device.
    Returns (attn_hard int16 [B,M,L], dur int64 [B,L] | None, path int16 [B,M] | None)."""
    _dev(logits, text_len, mel_len)
    assert logits.dtype == torch.float32 and logits.ndim == 3
    if logits.stride(2) != 1:
        logits = logits.contiguous()
    B, M, L = logits.shape
    text_len = text_len.to(torch.int64).contiguous()
    mel_len = mel_len.to(torch.int64).contiguous()
    hard = torch.empty((B, M, L), dtype=torch.int16, device=logits.device)
    dur = torch.empty((B, L), dtype=torch.int64, device=logits.device) if want_dur else None
    path = torch.empty((B, M), dtype=torch.int16, device=logits.device) if want_path else None
    _launch(f"mas_kernel<{(L + 63) // 64}>", 0.0, 6.0 * B * M * L, lib().ispk_mas_f32, logits.data_ptr(),
            text_len.data_ptr(), mel_len.data_ptr(), hard.data_ptr(), _ptr(dur), _ptr(path), B, M, L, logits.stride(0),
            logits.stride(1), _stream())
    return hard, dur, path


# ------------------------------------------------------------------------------------------------- LayerNorm
def layernorm(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], ada_scale: Optional[Tensor] = None,
              ada_shift: Optional[Tensor] = None, rows_per_batch: int = 1, row_mask: Optional[Tensor] = None,
              eps: float = 1e-5, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_layernorm_f32[_bf16].  x fp32 [..., D]; ada_* [Bc, D] with Bc == batch or 1 (broadcast)."""
    _dev(x, gamma, beta, ada_scale, ada_shift, row_mask)
    assert x.dtype == torch.float32
    x2 = _rows2d(x)
    rows, D = x2.shape
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    ada_stride = 0
    if ada_scale is not None:   # [Bc, D] rows, possibly column slices of one wide projection (row stride kept, no copy)
        ada_scale = ada_scale.reshape(-1, D) if ada_scale.ndim != 2 else ada_scale
        if ada_scale.stride(1) != 1:
            ada_scale = ada_scale.contiguous()
        if ada_shift is not None:
            ada_shift = ada_shift.reshape(-1, D) if ada_shift.ndim != 2 else ada_shift
            if ada_shift.stride(1) != 1 or ada_shift.stride(0) != ada_scale.stride(0):
                ada_scale, ada_shift = ada_scale.contiguous(), ada_shift.contiguous()
        ada_stride = ada_scale.stride(0) if ada_scale.shape[0] > 1 else 0
    if row_mask is not None:
        row_mask = row_mask.reshape(-1).contiguous()
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    fn = lib().ispk_layernorm_f32 if out_dtype == torch.float32 else lib().ispk_layernorm_f32_bf16
    label = f"layernorm_vec_kernel<{D // 128}>" if D % 128 == 0 and D <= 512 else f"layernorm_kernel<{D // 64}>"
    _launch(label, 0.0, float(rows) * D * (4 + y.element_size()), fn, x2.data_ptr(),
            x2.stride(0), _ptr(gamma), _ptr(beta), _ptr(ada_scale), _ptr(ada_shift), ada_stride, rows_per_batch,
            _ptr(row_mask), y.data_ptr(), D, rows, D, eps, _stream())
    return y


# ------------------------------------------------------------------------------------------------- GEMM
def _splitk_layout_ok(c2: Tensor, bias: Optional[Tensor], r2: Optional[Tensor], flags: int) -> bool:
    """The pointer / leading-dimension half of vec_epilogue_ok (csrc/gemm.hip), which ispk_gemm_bf16_splitk requires on
    top of its plan (the plan sees only M, N, K and flags).  Views that fail it (an offset `out=`, a bias slice off 16 bytes,
    an odd row stride) go to ispk_gemm_bf16, whose other kernels take any layout."""
    c_align = 8 if flags & EP_OUT_BF16 else 16
    r_align = 8 if flags & EP_RESID_BF16 else 16
    return (c2.stride(0) % 4 == 0 and c2.data_ptr() % c_align == 0 and
            (r2 is None or (r2.stride(0) % 4 == 0 and r2.data_ptr() % r_align == 0)) and
            (bias is None or bias.data_ptr() % 16 == 0))


def gemm(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
         mask: Optional[Tensor] = None, flags: int = 0, out: Optional[Tensor] = None,
         out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """C[..., N] = epilogue(a[..., K] @ w[N, K]^T)  (ispk_gemm_f32 / ispk_gemm_bf16 by a.dtype)."""
    _dev(a, w, bias, resid, mask, out)
    a2 = _rows2d(a)
    M, K = a2.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.stride(1) == 1 and a.dtype == w.dtype
    bf16 = a.dtype == torch.bfloat16
    if out_dtype is None:
        out_dtype = torch.float32 if not bf16 else torch.bfloat16
    if out is None:
        out = torch.empty((*a.shape[:-1], N), dtype=out_dtype, device=a.device)
    c2 = out.view(-1, N)
    r2 = None
    if resid is not None:
        r2 = _rows2d(resid)
        assert r2.shape == (M, N)
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
        assert mask.dtype == torch.bool
    if M == 0:      # nothing to compute; the C entries would refuse the NULL data_ptr() torch gives an empty tensor
        return out
    if bf16:
        if out.dtype == torch.bfloat16:
            flags |= EP_OUT_BF16
        if r2 is not None and r2.dtype == torch.bfloat16:
            flags |= EP_RESID_BF16
        fn = lib().ispk_gemm_bf16
        ks = lib().ispk_gemm_bf16_splitk_plan(M, N, K, flags) if M < 2048 and K >= 512 else 1
        if ks > 1 and _splitk_layout_ok(c2, bias, r2, flags):
            # few rows, long K: K slices on separate workgroups + one combine pass (ispk_gemm_bf16_splitk)
            ws = torch.empty((ks * M * N,), dtype=torch.float32, device=a.device)
            _launch(f"gemm_bf16_splitk<{ks}>", 2.0 * M * N * K, _gemm_bytes(a2, w, out, r2) + 8.0 * ks * M * N, lib().ispk_gemm_bf16_splitk,
                    a2.data_ptr(), a2.stride(0), w.data_ptr(), w.stride(0), c2.data_ptr(), c2.stride(0), _ptr(bias), _ptr(r2),
                    r2.stride(0) if r2 is not None else 0, _ptr(mask), M, N, K, flags, ws.data_ptr(), ks, _stream())
            return out
    else:
        assert out.dtype == torch.float32 and (r2 is None or r2.dtype == torch.float32)
        fn = lib().ispk_gemm_f32
    _launch(_gemm_label(bf16, M, N, K), 2.0 * M * N * K, _gemm_bytes(a2, w, out, r2), fn, a2.data_ptr(), a2.stride(0),
            w.data_ptr(), w.stride(0), c2.data_ptr(), c2.stride(0), _ptr(bias), _ptr(r2),
            r2.stride(0) if r2 is not None else 0, _ptr(mask), M, N, K, flags, 0, 0, _stream())
    return out


def ffn_pack_w2(w2: Tensor) -> Tensor:
    """ispk_ffn_pack_w2_bf16: W2 bf16 [D, inner] -> packed [inner/32, D, 32] (one-time weight staging for ffn_fused)."""
    _dev(w2)
    assert w2.dtype == torch.bfloat16 and w2.dim() == 2 and w2.stride(1) == 1
    D, Fi = w2.shape
    out = torch.empty((Fi // 32, D, 32), dtype=torch.bfloat16, device=w2.device)
    _launch("ffn_pack_w2_kernel", 0.0, 4.0 * D * Fi, lib().ispk_ffn_pack_w2_bf16, w2.data_ptr(), w2.stride(0), D, Fi,
            out.data_ptr(), _stream())
    return out


def ffn_fused(x: Tensor, w1: Tensor, w2: Tensor, resid: Optional[Tensor] = None, mask: Optional[Tensor] = None,
              bias1: Optional[Tensor] = None, bias2: Optional[Tensor] = None, flags: int = 0) -> Tensor:
    """ispk_ffn_bf16: out fp32 [..., D] = [mask] * (resid + gelu(x @ w1^T + bias1) @ w2^T + bias2), x / w1 / w2 bf16.
    w2 is either [D, inner] (nn.Linear layout) or the 3-D packed image from `ffn_pack_w2` (faster)."""
    _dev(x, w1, w2, resid, mask, bias1, bias2)
    assert x.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16
    x2 = _rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert w1.shape == (Fi, D) and w1.stride(1) == 1
    packed = w2.dim() == 3
    if packed:
        assert w2.shape == (Fi // 32, D, 32) and w2.is_contiguous()
    else:
        assert w2.shape == (D, Fi) and w2.stride(1) == 1
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    r2 = _rows2d(resid) if resid is not None else None
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
    nb = x2.numel() * 2 + (w1.numel() + w2.numel()) * 2 + out.numel() * 4 + (r2.numel() * 4 if r2 is not None else 0)
    _launch(f"ffn_bf16_kernel<{D // 64}>", 4.0 * R * D * Fi, float(nb), lib().ispk_ffn_bf16, x2.data_ptr(), x2.stride(0),
            w1.data_ptr(), w1.stride(0), _ptr(bias1), w2.data_ptr(), 0 if packed else w2.stride(0), _ptr(bias2), _ptr(r2),
            r2.stride(0) if r2 is not None else 0, _ptr(mask), out.data_ptr(), D, R, D, Fi, flags, _stream())
    return out


def ffn_prenorm(x: Tensor, norm_weight: Tensor, norm_bias: Tensor, w1: Tensor, w2p: Tensor, mask: Optional[Tensor] = None,
                bias2: Optional[Tensor] = None, flags: int = 0, norm_eps: float = 1e-5, want_stats: bool = False,
                stats_eps: float = 1e-5):
    """ispk_ffn_bf16_prenorm: out fp32 [..., D] = [mask] * (x + gelu(LN(x) @ w1^T) @ w2^T + bias2) from the fp32 rows x
    (LayerNorm input AND residual); with `want_stats` also the (mean, rstd) of the output rows, fp32 [rows, 2]."""
    _dev(x, norm_weight, norm_bias, w1, w2p, mask, bias2)
    assert x.dtype == torch.float32 and w1.dtype == torch.bfloat16 and w2p.dtype == torch.bfloat16
    x2 = _rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert w1.shape == (Fi, D) and w1.stride(1) == 1 and w2p.shape == (Fi // 32, D, 32) and w2p.is_contiguous()
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    stats = torch.empty((R, 2), dtype=torch.float32, device=x.device) if want_stats else None
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
    nb = x2.numel() * 8 + (w1.numel() + w2p.numel()) * 2 + out.numel() * 4 + (R * 8 if want_stats else 0)
    _launch(f"ffn_bf16_kernel<{D // 64}>", 4.0 * R * D * Fi, float(nb), lib().ispk_ffn_bf16_prenorm, x2.data_ptr(),
            x2.stride(0), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w1.stride(0),
            w2p.data_ptr(), _ptr(bias2), _ptr(mask), out.data_ptr(), D, R, D, Fi, flags, _ptr(stats), stats_eps, _stream())
    return (out, stats) if want_stats else out


def ffn_chunk_w2(w2: Tensor) -> Tensor:
    """ispk_ffn_chunk_w2_bf16: W2 bf16 [D, inner] -> chunk-contiguous [inner/32, D, 32] (weight staging for ffn_prenorm2)."""
    _dev(w2)
    assert w2.dtype == torch.bfloat16 and w2.dim() == 2 and w2.stride(1) == 1
    D, Fi = w2.shape
    out = torch.empty((Fi // 32, D, 32), dtype=torch.bfloat16, device=w2.device)
    _launch("ffn_chunk_w2_kernel", 0.0, 4.0 * D * Fi, lib().ispk_ffn_chunk_w2_bf16, w2.data_ptr(), w2.stride(0), D, Fi,
            out.data_ptr(), _stream())
    return out


def ffn_prenorm2(x: Tensor, norm_weight: Tensor, norm_bias: Tensor, w1: Tensor, w2c: Tensor, mask: Optional[Tensor] = None,
                 flags: int = 0, norm_eps: float = 1e-5, want_stats: bool = False, stats_eps: float = 1e-5):
    """ispk_ffn_bf16_prenorm2 (dim 384, eight-wave kernel): out fp32 [..., D] = [mask] * (x + gelu(LN(x) @ w1^T) @ w2^T) from the
    fp32 rows x; with `want_stats` also the (mean, rstd) of the output rows, fp32 [rows, 2].  w2c = `ffn_chunk_w2(w2)`."""
    _dev(x, norm_weight, norm_bias, w1, w2c, mask)
    assert x.dtype == torch.float32 and w1.dtype == torch.bfloat16 and w2c.dtype == torch.bfloat16
    x2 = _rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert w1.shape == (Fi, D) and w1.is_contiguous() and w2c.shape == (Fi // 32, D, 32) and w2c.is_contiguous()
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    stats = torch.empty((R, 2), dtype=torch.float32, device=x.device) if want_stats else None
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
    nb = x2.numel() * 8 + (w1.numel() + w2c.numel()) * 2 + out.numel() * 4 + (R * 8 if want_stats else 0)
    _launch("ffn2_bf16_kernel<0>", 4.0 * R * D * Fi, float(nb), lib().ispk_ffn_bf16_prenorm2, x2.data_ptr(),
            x2.stride(0), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(), _ptr(mask),
            out.data_ptr(), D, R, D, Fi, flags, _ptr(stats), stats_eps, _stream())
    return (out, stats) if want_stats else out


def chunk_k16(w: Tensor) -> Tensor:
    """ispk_chunk_k16_bf16: W bf16 [N, K] -> k-step chunks [K/16, N, 16] (weight staging for attn_out_ffn's q/kv epilogue)."""
    _dev(w)
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    out = torch.empty((K // 16, N, 16), dtype=torch.bfloat16, device=w.device)
    _launch("chunk_k16_kernel", 0.0, 4.0 * N * K, lib().ispk_chunk_k16_bf16, w.data_ptr(), w.stride(0), N, K, out.data_ptr(),
            _stream())
    return out


def attn_out_ffn(x: Tensor, attn_out: Tensor, woc: Tensor, norm_weight: Tensor, norm_bias: Tensor, w1: Tensor, w2c: Tensor,
                 mask: Optional[Tensor] = None, norm_eps: float = 1e-5, want_stats: bool = False, stats_eps: float = 1e-5,
                 next_qkv: Optional[tuple] = None, final_norm: Optional[tuple] = None, want_out: bool = True):
    """ispk_attn_out_ffn_bf16 (dim 384 = heads * 64): the second half of a pre-norm layer in one kernel,
        x1 = x + [mask] * (attn_out @ Wo^T);  out = [mask] * (x1 + gelu(LN(x1) @ w1^T) @ w2^T)
    from the fp32 residual rows x and the bf16 attention output; woc = `ffn_chunk_w2(Wo)`, w2c = `ffn_chunk_w2(w2)`.  With
    `want_stats` also the (mean, rstd) of the output rows, fp32 [rows, 2].  With `next_qkv` = (norm weight, norm bias, eps,
    `chunk_k16([Wq; Wkv])`) of the NEXT layer (ispk_attn_out_ffn_qkv_bf16) also that layer's q/kv rows, bf16 [..., 512]:
    -> (out, qkv).  With `final_norm` = (weight, bias, eps, apply_mask, dtype) of the STACK's final LayerNorm
    (ispk_attn_out_ffn_norm_bf16) also LN_final(out) [* mask]: -> (out | None, ln); `want_out=False` does not store the raw rows."""
    _dev(x, attn_out, woc, norm_weight, norm_bias, w1, w2c, mask)
    assert x.dtype == torch.float32 and attn_out.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16
    assert woc.dtype == torch.bfloat16 and w2c.dtype == torch.bfloat16
    x2, o2 = _rows2d(x), _rows2d(attn_out)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert o2.shape == (R, D) and woc.shape == (D // 32, D, 32) and woc.is_contiguous()
    assert w1.shape == (Fi, D) and w1.is_contiguous() and w2c.shape == (Fi // 32, D, 32) and w2c.is_contiguous()
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    stats = torch.empty((R, 2), dtype=torch.float32, device=x.device) if want_stats else None
    flags = 0
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
        flags = EP_MASK_ACC | EP_MASK_OUT
    nb = x2.numel() * 4 + o2.numel() * 2 + (woc.numel() + w1.numel() + w2c.numel()) * 2 + out.numel() * 4 + (R * 8 if want_stats else 0)
    if final_norm is not None:
        assert not want_stats and next_qkv is None
        fw, fb, feps, fmask, fdtype = final_norm
        _dev(fw, fb)
        assert fdtype in (torch.float32, torch.bfloat16)
        ln = torch.empty(x.shape, dtype=fdtype, device=x.device)
        outp = out if want_out else None
        _launch("ffn2_bf16_kernel<50>", 4.0 * R * D * Fi + 2.0 * R * D * D,
                float(nb - (0 if want_out else out.numel() * 4) + ln.numel() * ln.element_size()), lib().ispk_attn_out_ffn_norm_bf16,
                x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(), norm_weight.data_ptr(), norm_bias.data_ptr(),
                norm_eps, w1.data_ptr(), w2c.data_ptr(), _ptr(mask), _ptr(outp), D, R, D, Fi, flags, fw.data_ptr(), fb.data_ptr(), feps,
                int(bool(fmask) and mask is not None), ln.data_ptr(), D, int(fdtype == torch.bfloat16), _stream())
        return outp, ln
    if next_qkv is not None:
        assert not want_stats
        ng, nbeta, neps, wqc = next_qkv
        _dev(ng, nbeta, wqc)
        assert wqc.dtype == torch.bfloat16 and wqc.shape == (D // 16, 512, 16) and wqc.is_contiguous()
        qkv = torch.empty((*x.shape[:-1], 512), dtype=torch.bfloat16, device=x.device)
        _launch("ffn2_bf16_kernel<51>", 4.0 * R * D * Fi + 2.0 * R * D * D + 2.0 * R * D * 512, float(nb + wqc.numel() * 2 + R * 1024),
                lib().ispk_attn_out_ffn_qkv_bf16, x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(),
                norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(), _ptr(mask), out.data_ptr(), D,
                R, D, Fi, flags, ng.data_ptr(), nbeta.data_ptr(), neps, wqc.data_ptr(), qkv.data_ptr(), 512, _stream())
        return out, qkv
    _launch("ffn2_bf16_kernel<50>", 4.0 * R * D * Fi + 2.0 * R * D * D, float(nb), lib().ispk_attn_out_ffn_bf16, x2.data_ptr(),
            x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps,
            w1.data_ptr(), w2c.data_ptr(), _ptr(mask), out.data_ptr(), D, R, D, Fi, flags, _ptr(stats), stats_eps, _stream())
    return (out, stats) if want_stats else out


def ffn_prenorm2_split(x: Tensor, norm_weight: Tensor, norm_bias: Tensor, w1: Tensor, w2c: Tensor, mask: Optional[Tensor],
                       splits: int, next_norm: Optional[tuple] = None, norm_eps: float = 1e-5, attn_proj: Optional[tuple] = None):
    """Small-batch form of `ffn_prenorm2` (ispk_ffn_bf16_prenorm2_split + ispk_ffn_combine_ln_f32): the inner dimension split
    over `splits` workgroups per row block, partial products added in split order with the residual and the mask, and -
    `next_norm` = (weight, bias, eps, apply_mask, dtype) - the LayerNorm that consumes the result from the same pass.
    -> (y fp32, LN(y) | None).
    `attn_proj` = (attention output bf16 [..., D], `ffn_chunk_w2(Wo)`): x is the layer's INPUT and every split first forms
    x1 = x + [mask] * (attn_out @ Wo^T) in its accumulators (ispk_attn_out_ffn_split_bf16; split 0's partial product carries x1,
    the combine pass runs without a residual): y = [mask] * (x1 + feed_forward(LN(x1)))."""
    _dev(x, norm_weight, norm_bias, w1, w2c, mask)
    assert x.dtype == torch.float32 and w1.dtype == torch.bfloat16 and w2c.dtype == torch.bfloat16
    x2 = _rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    parts = torch.empty((splits, R, D), dtype=torch.float32, device=x.device)   # per call: graph instances may run side by side
    if attn_proj is not None:
        o, woc = attn_proj
        _dev(o, woc)
        o2 = _rows2d(o)
        assert o.dtype == torch.bfloat16 and o2.shape == (R, D) and woc.dtype == torch.bfloat16 and woc.shape == (D // 32, D, 32)
        mflat = mask.reshape(-1).contiguous() if mask is not None else None
        _launch("ffn2_bf16_kernel<21>", (4.0 * R * D * Fi) + 2.0 * R * D * D * splits,
                float((x2.numel() * 4 + o2.numel() * 2 + woc.numel() * 2) * splits + (w1.numel() + w2c.numel()) * 2 + splits * R * D * 4),
                lib().ispk_attn_out_ffn_split_bf16, x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(),
                norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(), _ptr(mflat),
                EP_MASK_ACC if mflat is not None else 0, parts.data_ptr(), R * D, splits, R, D, Fi, _stream())
    else:
        nbytes = x2.numel() * 4 * splits + (w1.numel() + w2c.numel()) * 2 + splits * R * D * 4
        _launch("ffn2_bf16_kernel<20>", 4.0 * R * D * Fi, float(nbytes), lib().ispk_ffn_bf16_prenorm2_split, x2.data_ptr(),
                x2.stride(0), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(),
                parts.data_ptr(), R * D, splits, R, D, Fi, _stream())
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
    ln = None
    nw = nb = None
    neps, nmask, nbf16 = 1e-5, 0, 0
    if next_norm is not None:
        nw, nb, neps, apply_mask, ndtype = next_norm
        ln = torch.empty(x.shape, dtype=ndtype, device=x.device)
        nmask, nbf16 = int(bool(apply_mask) and mask is not None), int(ndtype == torch.bfloat16)
    _launch("ffn_combine_ln_kernel", 0.0, float(R * D * 4 * (2 + splits) + (R * D * ln.element_size() if ln is not None else 0)),
            lib().ispk_ffn_combine_ln_f32, None if attn_proj is not None else x2.data_ptr(), x2.stride(0), parts.data_ptr(), R * D,
            splits, _ptr(mask), y.data_ptr(),
            D, _ptr(nw), _ptr(nb), neps, nmask, _ptr(ln), D, nbf16, R, D, _stream())
    return y, ln


def gemm_lnin(x: Tensor, stats: Optional[Tensor], ln_weight: Tensor, ln_bias: Tensor, w: Tensor,
              bias: Optional[Tensor] = None, mask: Optional[Tensor] = None, flags: int = 0,
              out_dtype: torch.dtype = torch.bfloat16, ln_eps: float = 1e-5) -> Tensor:
    """ispk_gemm_bf16_lnin: C[..., N] = epilogue(bf16(LayerNorm(x)) @ w[N, K]^T) with x fp32 [..., K]; the rows'
    (mean, rstd) come from `stats` (written by `ffn_prenorm` / `ffn_prenorm2`) or, with stats None, are computed by
    the kernel itself."""
    _dev(x, stats, ln_weight, ln_bias, w, bias, mask)
    assert x.dtype == torch.float32 and w.dtype == torch.bfloat16
    x2 = _rows2d(x)
    M, K = x2.shape
    N = w.shape[0]
    assert w.shape == (N, K) and w.stride(1) == 1
    assert stats is None or (stats.dtype == torch.float32 and stats.shape == (M, 2) and stats.is_contiguous())
    if out_dtype == torch.bfloat16:
        flags |= EP_OUT_BF16
    out = torch.empty((*x.shape[:-1], N), dtype=out_dtype, device=x.device)
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
    nb = x2.numel() * 4 + (stats.numel() * 4 if stats is not None else 0) + w.numel() * 2 + out.numel() * out.element_size()
    _launch(f"gemm_bf16_panel_kernel<{K // 64},lnin>", 2.0 * M * N * K, float(nb), lib().ispk_gemm_bf16_lnin, x2.data_ptr(),
            x2.stride(0), _ptr(stats), ln_weight.data_ptr(), ln_bias.data_ptr(), ln_eps, w.data_ptr(), w.stride(0),
            out.data_ptr(), N, _ptr(bias), 0, 0, _ptr(mask), M, N, K, flags, _stream())
    return out


def _gemm_label(bf16: bool, M: int, N: int, K: int) -> str:
    if bf16:
        return "gemm_bf16_kernel"
    t = lib().ispk_gemm_f32_tile(M, N, K)
    return f"gemm_f32_kernel<{t // 10},{t % 10}>"


def _gemm_bytes(a2: Tensor, w: Tensor, out: Tensor, r2: Optional[Tensor]) -> float:
    n = a2.numel() * a2.element_size() + w.numel() * w.element_size() + out.numel() * out.element_size()
    return float(n + (r2.numel() * r2.element_size() if r2 is not None else 0))


def to_mel(dec: Tensor, weight: Tensor, bias: Tensor, mask: Optional[Tensor]) -> Tensor:
    """mel[B, C, T] = mask[b,t] * (dec[B,T,D] @ weight[C,D]^T + bias[C])  — Linear + transpose + mask of
    model.py:167-168 as ONE GEMM with swapped operands: lanes run along the mel-frame axis T, so the transposed
    output is written with coalesced 128-B segments."""
    _dev(dec, weight, bias, mask)
    B, T, D = dec.shape
    C = weight.shape[0]
    x2 = _rows2d(dec)
    out = torch.empty((B, C, T), dtype=torch.float32, device=dec.device)
    if dec.dtype == torch.bfloat16 and D in (256, 384) and C % 4 == 0 and bias is not None:
        # bf16, K = 256 / 384: the panel GEMM with frames as rows and the transposed per-batch store (ISPK_EP_ROWS_T)
        flags = EP_ROWS_T
        if mask is not None:
            mask = mask.reshape(-1).contiguous()
            flags |= EP_MASK_OUT
        _launch("gemm_bf16_kernel", 2.0 * C * B * T * D, _gemm_bytes(x2, weight, out, None), lib().ispk_gemm_bf16,
                x2.data_ptr(), x2.stride(0), weight.data_ptr(), weight.stride(0), out.data_ptr(), T, _ptr(bias), None, 0,
                _ptr(mask), B * T, C, D, flags, T, C * T, _stream())
        return out
    flags = EP_BIAS_ROW | EP_MASK_COL
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
        flags |= EP_MASK_OUT
    fn = lib().ispk_gemm_bf16 if dec.dtype == torch.bfloat16 else lib().ispk_gemm_f32
    _launch(_gemm_label(dec.dtype == torch.bfloat16, C, B * T, D), 2.0 * C * B * T * D, _gemm_bytes(x2, weight, out, None),
            fn, weight.data_ptr(), weight.stride(0), x2.data_ptr(), x2.stride(0), out.data_ptr(), T, _ptr(bias), None, 0,
            _ptr(mask), C, B * T, D, flags, T, C * T, _stream())
    return out


def linear_small(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
                 act: int = 0) -> Tensor:
    """ispk_linear_small_f32: any K / N, fp32.  `w` may be a column slice of a wider weight (stride kept)."""
    _dev(a, w, bias, resid)
    assert a.dtype == torch.float32 and w.dtype == torch.float32 and w.stride(1) == 1
    a2 = _rows2d(a)
    M, K = a2.shape
    N = w.shape[0]
    assert w.shape[1] == K
    out = torch.empty((*a.shape[:-1], N), dtype=torch.float32, device=a.device)
    r2 = _rows2d(resid) if resid is not None else None
    _launch("linear_small_kernel", 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N), lib().ispk_linear_small_f32,
            a2.data_ptr(), a2.stride(0), w.data_ptr(), w.stride(0), _ptr(bias), _ptr(r2),
            r2.stride(0) if r2 is not None else 0, out.data_ptr(), N, M, N, K, act, _stream())
    return out


def linear(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, act: int = 0) -> Tensor:
    """nn.Linear on the device: MFMA GEMM when the shape allows (K % 8 == 0, enough rows), else the small kernel."""
    K = w.shape[1]
    rows = a.numel() // K
    if a.dtype == torch.float32 and (K % 8 != 0 or rows * w.shape[0] < 64 * 64 or w.stride(0) % 4 != 0
                                     or w.data_ptr() % 16 != 0):
        return linear_small(a, w, bias, None, act)
    return gemm(a, w, bias=bias, flags=act)


# ------------------------------------------------------------------------------------------------- attention
def alibi_mqa_attention_raw(q: Tensor, ldq: int, k: Tensor, v: Tensor, ldkv: int, slopes: Tensor,
                            key_len: Optional[Tensor], B: int, N: int, heads: int, q_tiles: int = 0) -> Tensor:
    """ispk_alibi_mqa_attn_*: q is any tensor whose storage holds [B][N][H*64] rows at leading stride ldq starting at
    q.data_ptr(); k / v likewise [B][N][64] at stride ldkv.  Returns the merged heads [B, N, H*64]."""
    _dev(q, k, v, slopes, key_len)
    out = torch.empty((B, N, heads * 64), dtype=q.dtype, device=q.device)
    if B == 0:      # nothing to compute; the C entries would refuse the NULL data_ptr() torch gives an empty tensor
        return out
    if key_len is not None:
        key_len = key_len.to(torch.int64).contiguous()
    slopes = slopes.to(torch.float32).contiguous()
    es = q.element_size()
    if es == 4:
        label = "attn_f32_kernel" + ("<384,16>" if heads <= 3 else "<768>" if heads <= 6 else "<1024>")
    else:
        label = "attn_bf16_kernel" + ("<768>" if heads <= 6 else "<1024>")
    flops, nbytes = 256.0 * B * N * N * heads, float(B) * N * (2 * heads * 64 + 128) * es
    if q_tiles:   # explicit query tiles per workgroup (bf16 kernel only; 0 = the launcher's own choice)
        assert es == 2
        _launch(label, flops, nbytes, lib().ispk_alibi_mqa_attn_bf16_tiles, q.data_ptr(), ldq, k.data_ptr(), v.data_ptr(),
                ldkv, slopes.data_ptr(), _ptr(key_len), out.data_ptr(), heads * 64, B, N, heads, q_tiles, _stream())
        return out
    fn = lib().ispk_alibi_mqa_attn_f32 if es == 4 else lib().ispk_alibi_mqa_attn_bf16
    _launch(label, flops, nbytes, fn, q.data_ptr(), ldq, k.data_ptr(), v.data_ptr(), ldkv,
            slopes.data_ptr(), _ptr(key_len), out.data_ptr(), heads * 64, B, N, heads, _stream())
    return out


def alibi_mqa_attention(qkv: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor], q_tiles: int = 0) -> Tensor:
    """qkv [B, N, H*64 + 128] = [Q | K | V] (the fused to_q / to_kv projection) -> merged heads [B, N, H*64]."""
    B, N, W = qkv.shape
    assert W == heads * 64 + 128 and qkv.is_contiguous()
    return alibi_mqa_attention_raw(qkv, W, qkv[..., heads * 64:], qkv[..., heads * 64 + 64:], W, slopes, key_len, B, N,
                                   heads, q_tiles)


# ------------------------------------------------------------------------------------------------- split-fp16 (parity-grade fast path)
# A "split" tensor is a torch.float16 tensor [2, *shape]: plane 0 = hi = fp16(v), plane 1 = lo = fp16(v - hi).
def split_f16(x: Tensor) -> Tensor:
    """ispk_split_f16: fp32 [..., C] (unit inner stride) -> split planes fp16 [2, ..., C]."""
    _dev(x)
    assert x.dtype == torch.float32
    x2 = _rows2d(x)
    rows, cols = x2.shape
    out = torch.empty((2, *x.shape), dtype=torch.float16, device=x.device)
    _launch("split_f16_kernel", 0.0, 8.0 * rows * cols, lib().ispk_split_f16, x2.data_ptr(), x2.stride(0), out[0].data_ptr(),
            out[1].data_ptr(), cols, rows, cols, _stream())
    return out


def layernorm_split(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], ada_scale: Optional[Tensor] = None,
                    ada_shift: Optional[Tensor] = None, rows_per_batch: int = 1, row_mask: Optional[Tensor] = None,
                    eps: float = 1e-5) -> Tensor:
    """ispk_layernorm_f32_split: `layernorm` with the result as split planes fp16 [2, ..., D]."""
    _dev(x, gamma, beta, ada_scale, ada_shift, row_mask)
    assert x.dtype == torch.float32
    x2 = _rows2d(x)
    rows, D = x2.shape
    y = torch.empty((2, *x.shape), dtype=torch.float16, device=x.device)
    ada_stride = 0
    if ada_scale is not None:
        ada_scale = ada_scale.reshape(-1, D) if ada_scale.ndim != 2 else ada_scale
        if ada_scale.stride(1) != 1:
            ada_scale = ada_scale.contiguous()
        if ada_shift is not None:
            ada_shift = ada_shift.reshape(-1, D) if ada_shift.ndim != 2 else ada_shift
            if ada_shift.stride(1) != 1 or ada_shift.stride(0) != ada_scale.stride(0):
                ada_scale, ada_shift = ada_scale.contiguous(), ada_shift.contiguous()
        ada_stride = ada_scale.stride(0) if ada_scale.shape[0] > 1 else 0
    if row_mask is not None:
        row_mask = row_mask.reshape(-1).contiguous()
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    label = f"layernorm_vec_kernel<{D // 128},split>" if D % 128 == 0 and D <= 512 else f"layernorm_kernel<{D // 64},split>"
    _launch(label, 0.0, float(rows) * D * 8, lib().ispk_layernorm_f32_split, x2.data_ptr(), x2.stride(0), _ptr(gamma),
            _ptr(beta), _ptr(ada_scale), _ptr(ada_shift), ada_stride, rows_per_batch, _ptr(row_mask), y.data_ptr(), D,
            y.stride(0), rows, D, eps, _stream())
    return y


def _split_label(M: int, N: int, K: int) -> str:
    t = lib().ispk_gemm_split_f16_tile(M, N, K)
    return f"gemm_split_f16_kernel<{t // 100},{t // 10 % 10},{t % 10}>"


def gemm_split(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
               mask: Optional[Tensor] = None, flags: int = 0, out_split: bool = False) -> Tensor:
    """ispk_gemm_split_f16: epilogue(a @ w^T) with a = split planes [2, ..., K], w = split planes [2, N, K].
    Returns fp32 [..., N], or split planes [2, ..., N] with `out_split` (no residual)."""
    _dev(a, w, bias, resid, mask)
    assert a.dtype == torch.float16 and w.dtype == torch.float16 and a.shape[0] == 2 and w.ndim == 3 and w.shape[0] == 2
    assert a.is_contiguous() and w.is_contiguous()
    K, N = a.shape[-1], w.shape[1]
    assert w.shape[2] == K
    M = a[0].numel() // K
    lead = a.shape[1:-1]
    r2 = None
    if resid is not None:
        r2 = _rows2d(resid)
        assert r2.shape == (M, N) and r2.dtype == torch.float32 and not out_split
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
        assert mask.dtype == torch.bool
    if out_split:
        out = torch.empty((2, *lead, N), dtype=torch.float16, device=a.device)
        flags |= EP_OUT_SPLIT
        c_plane, nb_out = out.stride(0), 4.0 * M * N
    else:
        out = torch.empty((*lead, N), dtype=torch.float32, device=a.device)
        c_plane, nb_out = 0, 4.0 * M * N
    nb = 4.0 * M * K + 4.0 * N * K + nb_out + (4.0 * M * N if r2 is not None else 0.0)
    _launch(_split_label(M, N, K), 2.0 * M * N * K, nb, lib().ispk_gemm_split_f16, a.data_ptr(), K, a.stride(0), w.data_ptr(), K,
            w.stride(0), out.data_ptr(), N, c_plane, _ptr(bias), _ptr(r2), r2.stride(0) if r2 is not None else 0, _ptr(mask), M, N,
            K, flags, 0, 0, _stream())
    return out


def to_mel_split(dec: Tensor, w: Tensor, bias: Tensor, mask: Optional[Tensor]) -> Tensor:
    """mel[B, C, T] = mask * (dec @ w^T + bias) from split planes dec [2, B, T, D], w [2, C, D] (ISPK_EP_ROWS_T)."""
    _dev(dec, w, bias, mask)
    _, B, T, D = dec.shape
    C = w.shape[1]
    out = torch.empty((B, C, T), dtype=torch.float32, device=dec.device)
    flags = EP_ROWS_T
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
        flags |= EP_MASK_OUT
    _launch(_split_label(B * T, C, D), 2.0 * C * B * T * D, 4.0 * (B * T * D + C * D + B * C * T), lib().ispk_gemm_split_f16,
            dec.data_ptr(), D, dec.stride(0), w.data_ptr(), D, w.stride(0), out.data_ptr(), T, 0, _ptr(bias), None, 0, _ptr(mask),
            B * T, C, D, flags, T, C * T, _stream())
    return out


def conv5_padded_split(xpad: Tensor, w2d: Tensor, flags: int = 0) -> Tensor:
    """`conv5_padded` on split planes: xpad [2, B, T+4, C], w2d [2, O, k*C] -> fp32 [B, T+4, O] (row t = frame t)."""
    _dev(xpad, w2d)
    _, B, TP, C = xpad.shape
    _, O, K = w2d.shape
    taps = K // C
    assert taps * C == K and taps in (1, 5) and xpad.is_contiguous() and w2d.is_contiguous()
    out = torch.empty((B, TP, O), dtype=torch.float32, device=xpad.device)
    a_ptr = xpad.data_ptr() + (0 if taps == 5 else 2 * C * 2)   # k=1: frame t sits at padded row t+2
    M = B * TP - 4
    _launch(_split_label(M, O, K), 2.0 * M * O * K, 4.0 * (M * C + O * K + M * O), lib().ispk_gemm_split_f16, a_ptr, C,
            xpad.stride(0), w2d.data_ptr(), K, w2d.stride(0), out.data_ptr(), O, 0, None, None, 0, None, M, O, K, flags, 0, 0,
            _stream())
    return out


def alibi_mqa_attention_split(qkv: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor], out_split: bool = True) -> Tensor:
    """ispk_alibi_mqa_attn_split_f16: qkv fp32 [B, N, H*64 + 128] -> merged heads as split planes [2, B, N, H*64] (or fp32)."""
    _dev(qkv, slopes, key_len)
    B, N, W = qkv.shape
    assert W == heads * 64 + 128 and qkv.is_contiguous() and qkv.dtype == torch.float32
    if key_len is not None:
        key_len = key_len.to(torch.int64).contiguous()
    slopes = slopes.to(torch.float32).contiguous()
    if out_split:
        out = torch.empty((2, B, N, heads * 64), dtype=torch.float16, device=qkv.device)
        plane = out.stride(0)
    else:
        out = torch.empty((B, N, heads * 64), dtype=torch.float32, device=qkv.device)
        plane = 0
    if B == 0:      # (NULL data_ptr() of an empty tensor: see alibi_mqa_attention_raw)
        return out
    es = qkv.element_size()
    _launch("attn_split_f16_kernel", 256.0 * B * N * N * heads, float(B) * N * (2 * heads * 64 + 128) * 4,
            lib().ispk_alibi_mqa_attn_split_f16, qkv.data_ptr(), W, qkv.data_ptr() + heads * 64 * es,
            qkv.data_ptr() + (heads * 64 + 64) * es, W, slopes.data_ptr(), _ptr(key_len), out.data_ptr(), heads * 64, plane, B, N,
            heads, _stream())
    return out


# ------------------------------------------------------------------------------------------------- aligner front-end
def pad_rows(x: Tensor, lengths: Tensor, channel_first: bool = False, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_pad_rows_f32: [B,T,C] (or [B,C,T] with channel_first) -> masked, zero-padded channel-last [B,T+4,C]."""
    _dev(x, lengths)
    assert x.dtype == torch.float32 and x.ndim == 3
    if channel_first:
        B, C, T = x.shape
        sb, sc, st = x.stride()
    else:
        B, T, C = x.shape
        sb, st, sc = x.stride()
    lengths = lengths.to(torch.int64).contiguous()
    split = out_dtype == torch.float16      # split fp16 planes [2, B, T+4, C] (hi, lo): the split-fp16 GEMMs' operand format
    out = torch.empty((2, B, T + 4, C) if split else (B, T + 4, C), dtype=out_dtype, device=x.device)
    _launch("pad_rows_kernel", 0.0, 8.0 * B * T * C, lib().ispk_pad_rows_f32, x.data_ptr(), sb, st, sc,
            lengths.data_ptr(), out.data_ptr(), 2 if split else int(out_dtype == torch.bfloat16), B, T, C, _stream())
    return out


def conv5_padded(xpad: Tensor, w2d: Tensor, flags: int = 0) -> Tensor:
    """Conv1d(kernel k, padding (k-1)/2, no bias) over a padded channel-last buffer as ONE GEMM over overlapping rows.
    xpad [B, T+4, C]; w2d [O, k*C] (= conv.weight.permute(0,2,1).reshape(O, k*C)), k = 5 or 1.  Returns [B, T+4, O] whose
    row t (not t+2) of every utterance is frame t; the last 4 rows per utterance are scratch."""
    _dev(xpad, w2d)
    B, TP, C = xpad.shape
    O, K = w2d.shape
    taps = K // C
    assert taps * C == K and taps in (1, 5) and xpad.is_contiguous() and w2d.is_contiguous()
    assert xpad.dtype == w2d.dtype
    bf16 = xpad.dtype == torch.bfloat16
    out = torch.empty((B, TP, O), dtype=torch.float32, device=xpad.device)      # fp32 out on both paths
    a_ptr = xpad.data_ptr() + (0 if taps == 5 else 2 * C * xpad.element_size())  # k=1: frame t sits at padded row t+2
    M = B * TP - 4
    fn = lib().ispk_gemm_bf16 if bf16 else lib().ispk_gemm_f32
    _launch(_gemm_label(bf16, M, O, K), 2.0 * M * O * K, float(xpad.element_size()) * (M * C + O * K) + 4.0 * M * O, fn,
            a_ptr, C, w2d.data_ptr(), K, out.data_ptr(), O, None, None, 0, None, M, O, K, flags, 0, 0, _stream())
    return out


def masked_instnorm(y: Tensor, weight: Tensor, bias: Tensor, lengths: Tensor, eps: float = 1e-5,
                    out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_masked_instnorm_f32: conv output [B,T+4,C] (row t = frame t) -> normalised, masked, re-padded [B,T+4,C]."""
    _dev(y, weight, bias, lengths)
    B, TP, C = y.shape
    split = out_dtype == torch.float16      # split fp16 planes [2, B, T+4, C]
    out = torch.empty((2, *y.shape) if split else y.shape, dtype=out_dtype, device=y.device)
    lengths = lengths.to(torch.int64).contiguous()
    _launch("masked_instnorm_kernel", 0.0, 16.0 * B * TP * C, lib().ispk_masked_instnorm_f32, y.data_ptr(),
            weight.data_ptr(), bias.data_ptr(), lengths.data_ptr(), out.data_ptr(), 2 if split else int(out_dtype == torch.bfloat16), B,
            TP - 4, C, eps, _stream())
    return out


def aligner_scores(q_enc: Tensor, k_enc: Tensor, text_len: Tensor, mel_len: Tensor, M: int, L: int, fast: bool = False):
    """ispk_aligner_scores_f32: q_enc [B, M+4, 128], k_enc [B, L+4, 128] (row t = frame/token t) ->
    (attn_soft, attn_logits), both [B, M, L].  `fast`: ispk_aligner_scores_fast_f32 (bf16 compute path: split-bf16 score
    products, hardware exp / log)."""
    _dev(q_enc, k_enc, text_len, mel_len)
    B, D = q_enc.shape[0], q_enc.shape[2]
    logits = torch.empty((B, M, L), dtype=torch.float32, device=q_enc.device)
    soft = torch.empty((B, M, L), dtype=torch.float32, device=q_enc.device)
    text_len = text_len.to(torch.int64).contiguous()
    mel_len = mel_len.to(torch.int64).contiguous()
    _launch("aligner_scores_kernel<bf16x3>" if fast else "aligner_scores_kernel", 2.0 * B * M * L * D, 4.0 * B * (M * D + L * D + 2 * M * L),
            lib().ispk_aligner_scores_fast_f32 if fast else lib().ispk_aligner_scores_f32, q_enc.data_ptr(), q_enc.stride(0), k_enc.data_ptr(), k_enc.stride(0),
            text_len.data_ptr(), mel_len.data_ptr(), logits.data_ptr(), soft.data_ptr(), B, M, L, D, _stream())
    return soft, logits


def soft_average(attn_soft: Tensor, pitch: Tensor, energy: Tensor, duration: Optional[Tensor], text_len: Tensor) -> Tensor:
    """ispk_soft_average_f32 -> feats [B, L, 3] = (log1p(duration) - or 0 without durations -, pitch target, energy target)."""
    _dev(attn_soft, pitch, energy, duration, text_len)
    B, M, L = attn_soft.shape
    feats = torch.empty((B, L, 3), dtype=torch.float32, device=attn_soft.device)
    dur = None if duration is None else duration.to(torch.int64).contiguous()
    _launch("soft_average_kernel", 0.0, 4.0 * B * M * L, lib().ispk_soft_average_f32, attn_soft.contiguous().data_ptr(),
            pitch.contiguous().data_ptr(), energy.contiguous().data_ptr(), _ptr(dur),
            text_len.to(torch.int64).contiguous().data_ptr(), feats.data_ptr(), B, M, L, _stream())
    return feats


def flow_mix(x0: Tensor, x1: Tensor, t: Tensor, sigma: float):
    """ispk_flow_mix_f32 -> (x_t, flow), both [B, L, C] fp32."""
    _dev(x0, x1, t)
    B, L, C = x1.shape
    x0c, x1c, tc = x0.float().contiguous(), x1.float().contiguous(), t.float().contiguous()
    xt, flow = torch.empty_like(x1c), torch.empty_like(x1c)
    _launch("flow_mix_kernel", 0.0, 16.0 * B * L * C, lib().ispk_flow_mix_f32, x0c.data_ptr(), x1c.data_ptr(), tc.data_ptr(),
            float(sigma), xt.data_ptr(), flow.data_ptr(), B, L, C, _stream())
    return xt, flow


def flow_finish(pred_raw: Tensor, flow: Tensor, x0: Tensor, mask: Tensor):
    """ispk_flow_finish_f32 -> (pred [B,L,C], duration [B,L], loss_ratio [B], loss = mean(loss_ratio) 0-d)."""
    _dev(pred_raw, flow, x0, mask)
    B, L, C = pred_raw.shape
    assert mask.dtype == torch.bool and mask.shape == (B, L)
    pr, fl, x0c, mk = pred_raw.float().contiguous(), flow.contiguous(), x0.float().contiguous(), mask.contiguous()
    pred = torch.empty_like(pr)
    dur = torch.empty((B, L), dtype=torch.float32, device=pr.device)
    ratio = torch.empty((B,), dtype=torch.float32, device=pr.device)
    loss = torch.empty((), dtype=torch.float32, device=pr.device)
    _launch("flow_finish_kernel", 0.0, 20.0 * B * L * C, lib().ispk_flow_finish_f32, pr.data_ptr(), fl.data_ptr(),
            x0c.data_ptr(), mk.data_ptr(), pred.data_ptr(), dur.data_ptr(), ratio.data_ptr(), loss.data_ptr(), B, L, C,
            _stream())
    return pred, dur, ratio, loss


def flow_head(y: Tensor, norm_weight: Tensor, norm_bias: Tensor, norm_eps: float, weight: Tensor, bias: Tensor, flow: Tensor,
              x0: Tensor, mask: Tensor):
    """ispk_flow_head_f32: the predictor's final LayerNorm (row-masked) + 256 -> 3 linear_layer + `flow_finish` on the stack's raw
    output rows y [B, L, 256] -> (pred [B,L,3], duration [B,L], loss_ratio [B], loss 0-d), two launches instead of three."""
    _dev(y, norm_weight, norm_bias, weight, bias, flow, x0, mask)
    B, L, D = y.shape
    C = weight.shape[0]
    assert y.dtype == torch.float32 and y.stride(2) == 1 and y.stride(0) == L * y.stride(1) and weight.shape == (C, D) and weight.is_contiguous()
    assert mask.dtype == torch.bool and mask.shape == (B, L)
    fl, x0c, mk = flow.contiguous(), x0.float().contiguous(), mask.contiguous()
    pred = torch.empty((B, L, C), dtype=torch.float32, device=y.device)
    dur = torch.empty((B, L), dtype=torch.float32, device=y.device)
    ratio = torch.empty((B,), dtype=torch.float32, device=y.device)
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    ws = torch.empty((2 * B * ((L + 15) // 16),), dtype=torch.float32, device=y.device)
    _launch("flow_head_kernels", 0.0, 4.0 * B * L * D, lib().ispk_flow_head_f32, y.data_ptr(), y.stride(1), norm_weight.data_ptr(),
            norm_bias.data_ptr(), float(norm_eps), weight.data_ptr(), bias.data_ptr(), fl.data_ptr(), x0c.data_ptr(), mk.data_ptr(),
            pred.data_ptr(), dur.data_ptr(), ratio.data_ptr(), loss.data_ptr(), ws.data_ptr(), B, L, D, C, _stream())
    return pred, dur, ratio, loss


def flow_euler(x_t: Tensor, velocity: Tensor, dt: float, mask: Optional[Tensor] = None) -> Tensor:
    """ispk_flow_euler_f32: x_t + velocity * dt [* mask[..., None]] (one Euler step of the flow predictor's `infer`)."""
    _dev(x_t, velocity, mask)
    B, L, C = x_t.shape
    xc, vc = x_t.float().contiguous(), velocity.float().contiguous()
    out = torch.empty_like(xc)
    if mask is not None:
        mask = mask.contiguous()
        assert mask.dtype == torch.bool and mask.shape == (B, L)
    _launch("flow_euler_kernel", 0.0, 12.0 * B * L * C, lib().ispk_flow_euler_f32, xc.data_ptr(), vc.data_ptr(), float(dt),
            _ptr(mask), out.data_ptr(), B, L, C, _stream())
    return out


def infer_features(pred: Tensor, duration_target: Optional[Tensor], pitch_target: Optional[Tensor],
                   energy_target: Optional[Tensor], duration_factor: float = 1.0, pitch_factor: float = 1.0,
                   pitch_delta: float = 0.0, energy_factor: float = 1.0, energy_delta: float = 0.0, round_duration: bool = False):
    """ispk_infer_features_f32: pred [B, L, 3] -> (duration fp32 [B, L], features fp32 [B, L, 2]).  `round_duration` (hard
    durations): ispk_infer_features_round_f32, the predicted durations rounded half to even before the clamp."""
    _dev(pred, duration_target, pitch_target, energy_target)
    B, L, C = pred.shape
    assert C == 3 and pred.dtype == torch.float32
    pc = pred.contiguous()
    dur_f = dur_i = None
    if duration_target is not None:
        assert duration_target.shape == (B, L)
        if duration_target.dtype == torch.int64:
            dur_i = duration_target.contiguous()
        else:
            dur_f = duration_target.float().contiguous()
    pt = None if pitch_target is None else pitch_target.float().reshape(B, L).contiguous()
    et = None if energy_target is None else energy_target.float().reshape(B, L).contiguous()
    duration = torch.empty((B, L), dtype=torch.float32, device=pred.device)
    feats = torch.empty((B, L, 2), dtype=torch.float32, device=pred.device)
    _launch("infer_features_kernel<round>" if round_duration else "infer_features_kernel", 0.0, 24.0 * B * L,
            lib().ispk_infer_features_round_f32 if round_duration else lib().ispk_infer_features_f32, pc.data_ptr(), _ptr(dur_f), _ptr(dur_i),
            _ptr(pt), _ptr(et), float(duration_factor), float(pitch_factor), float(pitch_delta), float(energy_factor),
            float(energy_delta), duration.data_ptr(), feats.data_ptr(), B, L, _stream())
    return duration, feats


# ------------------------------------------------------------------------------------------------- between the stacks
def embed_tokens(text: Tensor, table: Tensor, text_len: Optional[Tensor] = None, want_mask: bool = True):
    """ispk_embed_tokens_f32: (emb fp32 [B,L,D], mask bool [B,L] | None) - nn.Embedding lookup + the key mask."""
    _dev(text, table, text_len)
    assert text.dtype == torch.int64 and text.ndim == 2 and table.dtype == torch.float32 and table.stride(1) == 1
    B, L = text.shape
    V, D = table.shape
    text = text.contiguous()
    emb = torch.empty((B, L, D), dtype=torch.float32, device=text.device)
    mask = torch.empty((B, L), dtype=torch.bool, device=text.device) if want_mask else None
    if text_len is not None:
        text_len = text_len.to(torch.int64).contiguous()
    _launch("embed_tokens_kernel", 0.0, 8.0 * B * L * D, lib().ispk_embed_tokens_f32, text.data_ptr(), table.data_ptr(),
            table.stride(0), V, _ptr(text_len), emb.data_ptr(), _ptr(mask), B, L, D, _stream())
    return emb, mask


def embed_tokens_qkv(text: Tensor, table: Tensor, qkv_table: Tensor, text_len: Optional[Tensor] = None, want_mask: bool = True):
    """ispk_embed_tokens_qkv: `embed_tokens` plus the first layer's q/kv rows gathered with the same ids from `qkv_table` (bf16
    [vocab, N]: attention_norm + [to_q; to_kv] of every table row) -> (emb fp32 [B,L,D], mask bool [B,L] | None, qkv bf16 [B,L,N])."""
    _dev(text, table, qkv_table, text_len)
    assert text.dtype == torch.int64 and text.ndim == 2 and table.dtype == torch.float32 and table.stride(1) == 1
    B, L = text.shape
    V, D = table.shape
    N = qkv_table.shape[1]
    assert qkv_table.dtype == torch.bfloat16 and qkv_table.shape == (V, N) and qkv_table.stride(1) == 1
    text = text.contiguous()
    emb = torch.empty((B, L, D), dtype=torch.float32, device=text.device)
    qkv = torch.empty((B, L, N), dtype=torch.bfloat16, device=text.device)
    mask = torch.empty((B, L), dtype=torch.bool, device=text.device) if want_mask else None
    if text_len is not None:
        text_len = text_len.to(torch.int64).contiguous()
    _launch("embed_tokens_qkv_kernel", 0.0, B * L * (8.0 * D + 4.0 * N), lib().ispk_embed_tokens_qkv, text.data_ptr(),
            table.data_ptr(), table.stride(0), V, _ptr(text_len), emb.data_ptr(), _ptr(mask), qkv_table.data_ptr(),
            qkv_table.stride(0), qkv.data_ptr(), B, L, D, N, _stream())
    return emb, mask, qkv


def _speaker_ids(speaker: Tensor, B: int):
    """-> (contiguous int64 ids, id_stride): `speaker` int64 [B, 1] (the collator's field, collator.py:59) = one id per utterance,
    or one element = one id for the whole batch (the notebook's `torch.tensor([id])`)."""
    assert speaker.dtype == torch.int64
    if speaker.numel() == 1:
        return speaker.contiguous(), 0
    if speaker.ndim == 2 and tuple(speaker.shape) == (B, 1):
        return speaker.contiguous(), 1
    raise ValueError(f"speaker of shape {tuple(speaker.shape)} does not broadcast against enc_out [B={B}, L, D] "
                     "(the reference takes [B, 1] ids or a single id)")


def add_speaker_(x: Tensor, table: Tensor, speaker: Tensor) -> Tensor:
    """ispk_add_speaker_f32: x [B, L, D] += table[speaker] in place, broadcast over L the way the reference's
    `enc_out + self.speaker_embedding(speaker)` broadcasts (model.py:205-207): `speaker` int64 [B, 1] (the collator's field,
    collator.py:59) = one id per utterance, or one element = one id for the whole batch (the notebook's `torch.tensor([id])`)."""
    _dev(x, table, speaker)
    assert x.dtype == torch.float32 and x.ndim == 3 and x.is_contiguous() and table.dtype == torch.float32 and table.stride(1) == 1
    B, L, D = x.shape
    assert table.shape[1] == D
    speaker, stride = _speaker_ids(speaker, B)
    _launch("add_speaker_kernel", 0.0, 8.0 * B * L * D, lib().ispk_add_speaker_f32, x.data_ptr(), table.data_ptr(), table.stride(0),
            table.shape[0], speaker.data_ptr(), stride, B, L, D, _stream())
    return x


def add_speaker(x: Tensor, table: Tensor, speaker: Tensor) -> Tensor:
    """ispk_add_speaker_out_f32: -> x [B, L, D] + table[speaker] in a new tensor, bit for bit what `add_speaker_` leaves in
    place; x is untouched (the teacher-forced forward: the aligner reads - and its backward keeps - the un-added tensor)."""
    _dev(x, table, speaker)
    assert x.dtype == torch.float32 and x.ndim == 3 and x.is_contiguous() and table.dtype == torch.float32 and table.stride(1) == 1
    B, L, D = x.shape
    assert table.shape[1] == D
    speaker, stride = _speaker_ids(speaker, B)
    out = torch.empty_like(x)
    _launch("add_speaker_out_kernel", 0.0, 8.0 * B * L * D, lib().ispk_add_speaker_out_f32, x.data_ptr(), out.data_ptr(),
            table.data_ptr(), table.stride(0), table.shape[0], speaker.data_ptr(), stride, B, L, D, _stream())
    return out


def speaker_grad(d_x: Tensor, speaker: Tensor, speakers: int, text_len: Optional[Tensor] = None, out: Optional[Tensor] = None,
                 accumulate: bool = False) -> Tensor:
    """ispk_speaker_grad_f32: d_x fp32 [B, L, D] -> d_table [speakers, D], row s the sum of d_x[b, :text_len[b]] over the
    utterances of speaker s (fixed order, no atomics); rows of absent speakers are zero.  `out` (contiguous [speakers, D]) is
    written, or - `accumulate` - added to."""
    _dev(d_x, speaker, text_len, out)
    assert d_x.dtype == torch.float32 and d_x.ndim == 3
    d_x = d_x.contiguous()
    B, L, D = d_x.shape
    speaker, stride = _speaker_ids(speaker, B)
    if text_len is not None:
        text_len = text_len.to(torch.int64).contiguous()
        assert text_len.numel() == B
    if out is None:
        assert not accumulate
        out = torch.empty((speakers, D), dtype=torch.float32, device=d_x.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (speakers, D) and out.stride(1) == 1
    ws = workspace(d_x.device, B * -(-L // 16) * D)
    _launch("speaker_grad_kernels", 1.0 * B * L * D, 4.0 * B * L * D + 4.0 * speakers * D, lib().ispk_speaker_grad_f32, d_x.data_ptr(),
            speaker.data_ptr(), stride, _ptr(text_len), ws.data_ptr(), ws.numel(), out.data_ptr(), out.stride(0), speakers, B, L, D,
            1 if accumulate else 0, _stream())
    return out


def time_embedding(t: Tensor, inv_freq: Tensor, freq_scale: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor) -> Tensor:
    """ispk_time_embedding_f32: t [...] -> [..., emb_dim] (sinusoid with the raw position, Linear, SiLU, Linear)."""
    _dev(t, inv_freq, freq_scale, w0, b0, w1, b1)
    tf = t.to(torch.float32).contiguous()
    E, H = w1.shape[0], inv_freq.numel()
    assert w0.shape == (E, 1 + 2 * H) and w1.shape == (E, E) and w0.is_contiguous() and w1.is_contiguous()
    out = torch.empty((*t.shape, E), dtype=torch.float32, device=t.device)
    _launch("time_embedding_kernel", 0.0, 0.0, lib().ispk_time_embedding_f32, tf.data_ptr(), tf.numel(), inv_freq.data_ptr(),
            freq_scale.data_ptr(), H, w0.data_ptr(), b0.data_ptr(), w1.data_ptr(), b1.data_ptr(), E, out.data_ptr(),
            _stream())
    return out


def length_regulate(x: Tensor, durations: Tensor, alignment: Optional[Tensor], frames: int, max_len: int = -1,
                    enc_len: Optional[Tensor] = None, want_mask: bool = True, split_bf16=False, next_qkv: Optional[tuple] = None):
    """ispk_length_regulate_f32 -> (out fp32 [B, frames, D], dec_len int64 [B], dec_mask bool [B, frames] | None).
    alignment fp32 [B, frames, L] (forward), or None: the soft path generated from the fp32 `durations` (infer).
    `split_bf16`: True = ispk_length_regulate_split_bf16 (the bf16 compute path: three bf16 MFMAs per product, ~2^-16
    relative); "f16" = ispk_length_regulate_split_f16 (the split-fp16 parity path: fp16 terms, fp32-grade).
    `next_qkv` = (gamma, beta, eps, Wqkv_chunks) (bf16 path, D = 384; Wqkv_chunks from `chunk_k16`, [24, 512, 16]):
    ispk_length_regulate_qkv_bf16 - the same three outputs, bit for bit, and a fourth: the consuming layer's attention_norm +
    q/kv projection of every output row, bf16 [B, frames, 512], from the kernel's epilogue."""
    _dev(x, durations, alignment, enc_len)
    assert x.dtype == torch.float32 and x.ndim == 3
    if x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        x = x.contiguous()
    B, L, D = x.shape
    if alignment is not None:
        assert alignment.dtype == torch.float32 and alignment.shape == (B, frames, L)
        alignment = alignment.contiguous()
    dur_f = dur_i = None
    dur_cols = L
    if durations.dtype == torch.int64:   # only summed: any [B, cols] with the right row sums (e.g. mel_len as [B, 1])
        assert alignment is not None, "the soft path is generated from fp32 durations"
        dur_i = durations.reshape(B, -1).contiguous()
        dur_cols = dur_i.shape[1]
    else:
        dur_f = durations.to(torch.float32).contiguous()
        assert dur_f.shape == (B, L)
    if enc_len is not None:
        enc_len = enc_len.to(torch.int64).contiguous()
    out = torch.empty((B, frames, D), dtype=torch.float32, device=x.device)
    dec_len = torch.empty((B,), dtype=torch.int64, device=x.device)
    mask = torch.empty((B, frames), dtype=torch.bool, device=x.device) if want_mask else None
    nb = 4.0 * B * (frames * D + L * D + (frames * L if alignment is not None else 0))
    if next_qkv is not None:
        gamma, beta, eps, wqc = next_qkv
        _dev(gamma, beta, wqc)
        assert split_bf16 is True and D == 384, "the q/kv epilogue is built for the bf16 path at dim 384"
        assert wqc.dtype == torch.bfloat16 and wqc.shape == (D // 16, 512, 16) and wqc.is_contiguous()
        assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == D
        qkv = torch.empty((B, frames, 512), dtype=torch.bfloat16, device=x.device)
        _launch("length_regulate_qkv_kernel", 2.0 * B * frames * (L + 512) * D, nb + 2.0 * (B * frames * 512 + 512 * D),
                lib().ispk_length_regulate_qkv_bf16, _ptr(alignment), _ptr(dur_f), _ptr(dur_i), _ptr(enc_len), x.data_ptr(),
                x.stride(1), out.data_ptr(), dec_len.data_ptr(), _ptr(mask), gamma.data_ptr(), beta.data_ptr(), float(eps),
                wqc.data_ptr(), qkv.data_ptr(), 512, B, frames, L, D, max_len, dur_cols, _stream())
        return out, dec_len, mask, qkv
    fn = (lib().ispk_length_regulate_split_f16 if split_bf16 == "f16" else
          lib().ispk_length_regulate_split_bf16 if split_bf16 else lib().ispk_length_regulate_f32)
    _launch("length_regulate_kernel<split_f16>" if split_bf16 == "f16" else "length_regulate_kernel<bf16x3>" if split_bf16
            else "length_regulate_kernel", 2.0 * B * frames * L * D, nb, fn, _ptr(alignment),
            _ptr(dur_f), _ptr(dur_i), _ptr(enc_len), x.data_ptr(), x.stride(1), out.data_ptr(), dec_len.data_ptr(),
            _ptr(mask), B, frames, L, D, max_len, dur_cols, _stream())
    return out, dec_len, mask


def _hard_durations(durations: Tensor, B: int, L: int):
    """-> (fp32 pointer source | None, int64 pointer source | None) of [B, L] durations: int64 (MAS) or fp32 (`infer`)."""
    assert durations.shape == (B, L), f"durations {tuple(durations.shape)}: one per token, [{B}, {L}]"
    if durations.dtype == torch.int64:
        return None, durations.contiguous()
    return durations.to(torch.float32).contiguous(), None


def hard_regulate(x: Tensor, durations: Tensor, frames: int, max_len: int = -1, want_mask: bool = True):
    """ispk_hard_regulate_f32 -> (out fp32 [B, frames, D], dec_len int64 [B], dec_mask bool [B, frames] | None): every token row
    of x [B, L, D] repeated (float(duration) + 0.5).long() times, zero rows behind the last one."""
    _dev(x, durations)
    assert x.dtype == torch.float32 and x.ndim == 3
    if x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        x = x.contiguous()
    B, L, D = x.shape
    dur_f, dur_i = _hard_durations(durations, B, L)
    out = torch.empty((B, frames, D), dtype=torch.float32, device=x.device)
    dec_len = torch.empty((B,), dtype=torch.int64, device=x.device)
    mask = torch.empty((B, frames), dtype=torch.bool, device=x.device) if want_mask else None
    _launch("hard_regulate_kernel", 0.0, 4.0 * B * D * (frames + L), lib().ispk_hard_regulate_f32, _ptr(dur_f), _ptr(dur_i),
            x.data_ptr(), x.stride(1), out.data_ptr(), dec_len.data_ptr(), _ptr(mask), B, frames, L, D, max_len, _stream())
    return out, dec_len, mask


def hard_regulate_bwd(d_out: Tensor, durations: Tensor, max_len: int = -1) -> Tensor:
    """ispk_hard_regulate_bwd_f32: d_out [B, rows, D] -> d_x [B, L, D], each token the sum of its frames' rows in frame order."""
    _dev(d_out, durations)
    assert d_out.dtype == torch.float32 and d_out.ndim == 3
    d_out = d_out.contiguous()
    B, rows, D = d_out.shape
    L = durations.shape[1]
    dur_f, dur_i = _hard_durations(durations, B, L)
    d_x = torch.empty((B, L, D), dtype=torch.float32, device=d_out.device)
    _launch("hard_regulate_bwd_kernel", 1.0 * B * rows * D, 4.0 * B * D * (rows + L), lib().ispk_hard_regulate_bwd_f32, _ptr(dur_f),
            _ptr(dur_i), d_out.data_ptr(), d_x.data_ptr(), B, rows, L, D, max_len, _stream())
    return d_x


def hard_average(pitch: Tensor, energy: Tensor, duration: Tensor, text_len: Tensor) -> Tensor:
    """ispk_hard_average_f32 -> feats [B, L, 3] = (log1p(duration), mean of each token's non-zero pitch frames, same for energy);
    pitch / energy fp32 [B, M], duration int64 [B, L]."""
    _dev(pitch, energy, duration, text_len)
    B, M = pitch.shape
    L = duration.shape[1]
    assert duration.dtype == torch.int64 and duration.shape == (B, L) and energy.shape == (B, M)
    feats = torch.empty((B, L, 3), dtype=torch.float32, device=pitch.device)
    # (copies of strided views stay referenced until the launch is queued: a freed one's block would be handed to the next copy)
    pc, ec, dc, tc = pitch.float().contiguous(), energy.float().contiguous(), duration.contiguous(), text_len.to(torch.int64).contiguous()
    _launch("hard_average_kernel", 0.0, 8.0 * B * M + 20.0 * B * L, lib().ispk_hard_average_f32, pc.data_ptr(), ec.data_ptr(),
            dc.data_ptr(), tc.data_ptr(), feats.data_ptr(), B, M, L, _stream())
    return feats


def cast_bf16(x: Tensor) -> Tensor:
    _dev(x)
    x2 = _rows2d(x)
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _launch("cast_bf16_kernel", 0.0, 6.0 * x2.numel(), lib().ispk_cast_f32_bf16, x2.data_ptr(), x2.stride(0),
            y.data_ptr(), x2.shape[1], x2.shape[0], x2.shape[1], _stream())
    return y


# ------------------------------------------------------------------------------------------------- data movement (csrc/util.hip)
class _Segment(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", ctypes.c_int64), ("mode", ctypes.c_int32)]


SEG_COPY, SEG_ADD, SEG_BF16 = 0, 1, 2


class _Stage(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("ld_dst", ctypes.c_int64), ("flags", ctypes.c_int32)]


stage_calls = 0     # how many staging passes have been launched (train/graph.py checks that a capture recorded one)


def stage_weights(items) -> None:
    """ispk_stage_weights: items = [(src fp32 contiguous [rows, cols], dst 2-D view with unit column stride (fp32 or bf16),
    transposed: bool, exp: bool)], 16 per launch.  dst is [rows, cols], or [cols, rows] when transposed."""
    global stage_calls
    if not items:
        return
    stage_calls += 1
    arr = (_Stage * len(items))()
    nbytes = 0.0
    for k, (src, dst, tr, ex) in enumerate(items):
        _dev(src, dst)
        src = src.detach()
        assert src.dtype == torch.float32 and src.ndim == 2 and src.is_contiguous() and dst.ndim == 2 and dst.stride(1) == 1
        assert tuple(dst.shape) == ((src.shape[1], src.shape[0]) if tr else tuple(src.shape)) and dst.dtype in (torch.float32, torch.bfloat16)
        arr[k].src, arr[k].dst, arr[k].rows, arr[k].cols = src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1]
        arr[k].ld_dst = dst.stride(0)
        arr[k].flags = (1 if tr else 0) | (2 if dst.dtype == torch.bfloat16 else 0) | (4 if ex else 0)
        nbytes += src.numel() * (4.0 + dst.element_size())
    _launch("stage_kernel", 0.0, nbytes, lib().ispk_stage_weights, ctypes.cast(arr, ctypes.c_void_p), len(items), _stream())


def segments(items) -> None:
    """ispk_segments_f32: items = [(src fp32 contiguous, dst contiguous view, mode)], any number, 32 per launch:
    SEG_COPY dst = src, SEG_ADD dst += src, SEG_BF16 dst(bf16) = src."""
    if not items:
        return
    arr = (_Segment * len(items))()
    nbytes = 0.0
    for k, (src, dst, mode) in enumerate(items):
        _dev(src, dst)
        assert src.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
        assert dst.dtype == (torch.bfloat16 if mode == SEG_BF16 else torch.float32)
        arr[k].src, arr[k].dst, arr[k].n, arr[k].mode = src.data_ptr(), dst.data_ptr(), src.numel(), mode
        nbytes += src.numel() * (4.0 + dst.element_size() * (2 if mode == SEG_ADD else 1))
    _launch("segments_kernel", 0.0, nbytes, lib().ispk_segments_f32, ctypes.cast(arr, ctypes.c_void_p), len(items), _stream())


def cat0(tensors, dtype: torch.dtype = torch.float32) -> Tensor:
    """torch.cat(tensors, 0).to(dtype) of contiguous fp32 tensors as one ispk_segments_f32 launch (weights that change every
    training step: the fused [to_q; to_kv] image, the adaptive norms' stacked projections)."""
    srcs = [t.detach() for t in tensors]
    assert dtype in (torch.float32, torch.bfloat16) and all(t.dtype == torch.float32 and t.is_contiguous() for t in srcs)
    rows = sum(t.shape[0] for t in srcs)
    out = torch.empty((rows, *srcs[0].shape[1:]), dtype=dtype, device=srcs[0].device)
    items, r = [], 0
    for t in srcs:
        items.append((t, out[r:r + t.shape[0]], SEG_BF16 if dtype == torch.bfloat16 else SEG_COPY))
        r += t.shape[0]
    segments(items)
    return out


def deliver_grads(pairs) -> list:
    """pairs = [(parameter, gradient | None)] -> the list of gradients to hand to autograd.  A gradient whose parameter's .grad
    is a buffer of an optimizer arena (`FlatParameters` marks it `_ispk_grad_arena`) is written - or added, if something has
    been delivered since the arena was zeroed - into it by ONE segments launch for the whole list, and autograd gets None:
    no AccumulateGrad add per parameter."""
    out, items, seen = [], [], set()
    for p, g in pairs:
        if g is not None and not p.requires_grad:
            # frozen AFTER the arena was built (model.freeze(), row f3): autograd would have dropped this gradient - so do we,
            # instead of writing it into the arena where AdamW would apply it
            out.append(None)
            continue
        buf = p.grad if g is not None else None
        if buf is not None and getattr(buf, "_ispk_grad_arena", False) and g.is_cuda:
            g = g.detach()
            g = g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()
            if buf.data_ptr() in seen:
                # the same parameter twice in one call: two segments of ONE launch writing one buffer would race - flush first
                segments(items)
                items, seen = [], set()
            seen.add(buf.data_ptr())
            items.append((g, buf, SEG_ADD if getattr(buf, "_ispk_dirty", False) else SEG_COPY))
            buf._ispk_dirty = True
            out.append(None)
        else:
            out.append(g)
    segments(items)
    return out


def zero_(t: Tensor) -> Tensor:
    """ispk_fill_zero on a contiguous tensor."""
    _dev(t)
    assert t.is_contiguous()
    _launch("fill_zero_kernel", 0.0, float(t.numel() * t.element_size()), lib().ispk_fill_zero, t.data_ptr(),
            t.numel() * t.element_size(), _stream())
    return t


def _zero_rows(out: Tensor) -> Tensor:
    """The result of a weight-gradient product over zero rows: `out` zeroed (a strided view: copied from a zeroed scratch)."""
    if out.numel() == 0 or out.is_contiguous():
        return zero_(out) if out.numel() else out
    z = zeros(tuple(out.shape[-2:]), device=out.device)
    for o in (out,) if out.ndim == 2 else out:
        copy2d(z, o)
    return out


def zeros(shape, dtype: torch.dtype = torch.float32, device=None) -> Tensor:
    return zero_(torch.empty(shape, dtype=dtype, device=device))


def scale_(x: Tensor, s_dev: Optional[Tensor] = None, s_host: float = 1.0) -> Tensor:
    """ispk_scale_f32: x *= s_dev[0] * s_host in place (s_dev: a one-element fp32 device tensor or None)."""
    _dev(x, s_dev)
    assert x.dtype == torch.float32 and x.is_contiguous() and (s_dev is None or (s_dev.dtype == torch.float32 and s_dev.numel() == 1))
    _launch("scale_kernel", 0.0, 8.0 * x.numel(), lib().ispk_scale_f32, x.data_ptr(), x.numel(), _ptr(s_dev), float(s_host), _stream())
    return x


def sum_scalars(terms, weights=None) -> Tensor:
    """ispk_sum_scalars_f32 -> 0-dim fp32: sum_i weights[i] * terms[i] (one-element fp32 device tensors), in index order."""
    terms = list(terms)
    _dev(*terms)
    assert 1 <= len(terms) <= 8 and all(t.dtype == torch.float32 and t.numel() == 1 for t in terms)
    ptrs = (ctypes.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
    ws = (ctypes.c_float * len(terms))(*([1.0] * len(terms) if weights is None else [float(w) for w in weights]))
    out = torch.empty((1,), dtype=torch.float32, device=terms[0].device)
    _launch("sum_scalars_kernel", 0.0, 0.0, lib().ispk_sum_scalars_f32, ctypes.cast(ptrs, ctypes.c_void_p),
            ctypes.cast(ws, ctypes.c_void_p), len(terms), out.data_ptr(), _stream())
    return out.reshape(())


def exp_pad(src: Tensor, total: Optional[int] = None) -> Tensor:
    """ispk_exp_pad_f32: exp(src) (fp32, flattened), zero-padded to `total` elements."""
    _dev(src)
    src = src.detach().reshape(-1)
    assert src.dtype == torch.float32 and src.is_contiguous()
    total = src.numel() if total is None else total
    out = torch.empty((total,), dtype=torch.float32, device=src.device)
    _launch("unary_kernel", 0.0, 0.0, lib().ispk_exp_pad_f32, src.data_ptr(), out.data_ptr(), src.numel(), total, _stream())
    return out


def sqrt_scale(src: Tensor, scale: float = 1.0) -> Tensor:
    """ispk_sqrt_scale_f32: sqrt(src) * scale (fp32)."""
    _dev(src)
    assert src.dtype == torch.float32 and src.is_contiguous()
    out = torch.empty_like(src)
    _launch("unary_kernel", 0.0, 0.0, lib().ispk_sqrt_scale_f32, src.data_ptr(), out.data_ptr(), src.numel(), float(scale), _stream())
    return out


def copy2d(src: Tensor, dst: Tensor) -> Tensor:
    """ispk_copy2d_f32: dst[:, :] = src for 2-D fp32 views with unit column stride."""
    _dev(src, dst)
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.ndim == 2 and src.shape == dst.shape
    assert src.stride(1) == 1 and dst.stride(1) == 1
    _launch("copy2d_kernel", 0.0, 8.0 * src.numel(), lib().ispk_copy2d_f32, src.data_ptr(), src.stride(0), dst.data_ptr(),
            dst.stride(0), src.shape[0], src.shape[1], _stream())
    return dst


def permute021(src: Tensor) -> Tensor:
    """ispk_permute021_f32: [A, B, C] fp32 contiguous -> contiguous [A, C, B]."""
    _dev(src)
    src = src.detach()
    assert src.dtype == torch.float32 and src.ndim == 3 and src.is_contiguous()
    A, B, C = src.shape
    out = torch.empty((A, C, B), dtype=torch.float32, device=src.device)
    _launch("permute021_kernel", 0.0, 8.0 * src.numel(), lib().ispk_permute021_f32, src.data_ptr(), out.data_ptr(), A, B, C, _stream())
    return out


def conv_weight_flip(w: Tensor) -> Tensor:
    """ispk_conv_weight_flip_f32: Conv1d weight [O, C, K] -> [C, K * O] with wf[c][(K-1-k) O + o] = w[o][c][k]."""
    _dev(w)
    w = w.detach()
    assert w.dtype == torch.float32 and w.ndim == 3 and w.is_contiguous()
    O, C, K = w.shape
    out = torch.empty((C, K * O), dtype=torch.float32, device=w.device)
    _launch("conv_flip_kernel", 0.0, 8.0 * w.numel(), lib().ispk_conv_weight_flip_f32, w.data_ptr(), out.data_ptr(), O, C, K, _stream())
    return out


def draw_seed() -> int:
    """A 62-bit seed for one launch group's dropout masks from torch's CPU generator (`torch.manual_seed(s)` reproduces a
    run): a host-side draw, no device tensor and no device round trip."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# ------------------------------------------------------------------------------------------------- training step (row f2)
def transpose(x: Tensor) -> Tensor:
    """ispk_transpose_f32: y[c, r] = x[r, c] (fp32 matrix; weights for dX = dY . W through the NT GEMM)."""
    _dev(x)
    assert x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1
    y = torch.empty((x.shape[1], x.shape[0]), dtype=torch.float32, device=x.device)
    _launch("transpose_kernel", 0.0, 8.0 * x.numel(), lib().ispk_transpose_f32, x.data_ptr(), x.stride(0), y.data_ptr(),
            y.stride(0), x.shape[0], x.shape[1], _stream())
    return y


_TN_WORKSPACE_FLOATS = 48 << 20     # 192 MB: up to 64+ row ranges of the largest weight (1536 x 384)
_workspaces: dict = {}


def drop_workspace(key) -> None:
    """Forget the scratch buffer of one (device index, stream) - a HIP graph's capture stream when the graph is destroyed."""
    _workspaces.pop(key, None)


def workspace(device, floats: int) -> Tensor:
    """Scratch for the backward kernels' partial sums, one buffer per (device, CURRENT STREAM): launches on one stream use it
    in order; a backward node that autograd runs on another stream (its forward ran there) gets its own buffer instead of
    racing on the partial sums.  Grown on demand, reused."""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream if torch.cuda.is_available() else 0)
    w = _workspaces.get(key)
    if w is None or w.numel() < floats:
        w = _workspaces[key] = torch.empty((max(floats, _TN_WORKSPACE_FLOATS),), dtype=torch.float32, device=device)
    return w


def gemm_tn(a: Tensor, b: Tensor, row_mask: Optional[Tensor] = None, out: Optional[Tensor] = None,
            accumulate: bool = False, bf16: bool = False) -> Tensor:
    """ispk_gemm_tn_f32: C[N1, N2] (+)= sum_m mask[m] a[m, N1] b[m, N2] - the weight gradient dY^T . X of a Linear.
    `bf16`: ispk_gemm_tn_bf16, the operands rounded to bf16 in flight (autocast's weight gradient), fp32 accumulation."""
    _dev(a, b, row_mask, out)
    a2, b2 = _rows2d(a), _rows2d(b)
    in16 = a2.dtype == torch.bfloat16
    assert a2.dtype == b2.dtype and a2.dtype in (torch.float32, torch.bfloat16) and a2.shape[0] == b2.shape[0]
    M, N1 = a2.shape
    N2 = b2.shape[1]
    if out is None:
        assert not accumulate
        out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
    assert out.shape == (N1, N2) and out.stride(1) == 1 and out.dtype == torch.float32
    if row_mask is not None:
        row_mask = row_mask.reshape(-1).contiguous()
        assert row_mask.dtype == torch.bool and row_mask.numel() == M
    if M == 0:      # a sum over no rows (the C entry refuses M = 0 and the NULL data_ptr() of an empty tensor)
        return out if accumulate else _zero_rows(out)
    ws = workspace(a.device, N1 * N2)
    # one row: the leading dimensions are never stepped, and torch reports a single row's stride as its width whatever the
    # view's real stride was (reshape), which the bf16 entry refuses for N % 8 == 4 - pass a width the ABI accepts
    lda, ldb = (a2.stride(0), b2.stride(0)) if M > 1 else (-(-N1 // 8) * 8, -(-N2 // 8) * 8)
    fn = lib().ispk_gemm_tn_b16 if in16 else (lib().ispk_gemm_tn_bf16 if bf16 else lib().ispk_gemm_tn_f32)
    _launch(f"gemm_tn_{'b16_' if in16 else ('bf16_' if bf16 else '')}kernel<{N1}x{N2}>", 2.0 * M * N1 * N2,
            float(a2.element_size()) * (a2.numel() + b2.numel()) + 4.0 * out.numel(), fn, a2.data_ptr(), lda, b2.data_ptr(), ldb, out.data_ptr(), out.stride(0), M,
            N1, N2, _ptr(row_mask), int(accumulate), ws.data_ptr(), ws.numel(), _stream())
    return out


def gemm_gelu_train(x: Tensor, w: Tensor, dropout_p: float = 0.0, seed: int = 0):
    """ispk_gemm_bf16_gelu_train -> (u, a): u = x @ w^T and a = dropout(gelu(u)), both bf16, from ONE launch (the first Linear
    of a feed-forward block in an AMP training step: `gemm(x, w)` followed by `gelu(u, dropout_p, seed)`, bit for bit).
    x bf16 [..., K], w bf16 [N, K], K = 256 / 384."""
    _dev(x, w)
    x2 = _rows2d(x)
    M, K = x2.shape
    N = w.shape[0]
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.shape[1] == K and w.stride(1) == 1
    u = torch.empty((*x.shape[:-1], N), dtype=torch.bfloat16, device=x.device)
    a = torch.empty_like(u)
    _launch(f"gemm_bf16_panel_kernel<{K // 64},gelu_train>", 2.0 * M * N * K, 2.0 * (M * K + N * K + 2 * M * N), lib().ispk_gemm_bf16_gelu_train,
            x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), u.data_ptr(), N, a.data_ptr(), N, M, N, K, dropout_p,
            seed & 0xFFFFFFFFFFFFFFFF, _stream())
    return u, a


def gemm_gelu_bwd(dy: Tensor, w2_t: Tensor, u: Tensor, mask: Optional[Tensor] = None, dropout_p: float = 0.0, seed: int = 0) -> Tensor:
    """ispk_gemm_bf16_gelu_bwd -> du = (mask dy @ w2_t^T) * gelu'(u) * [keep / (1 - p)] (bf16): the feed-forward backward's
    `gemm(dy, w2_t, mask=mask, flags=EP_MASK_OUT)` + `gelu_bwd(da, u, dropout_p=, seed=)` as ONE launch, bit for bit.
    dy bf16 [..., K], w2_t bf16 [N, K] (= W2^T rows), u bf16 [..., N]."""
    _dev(dy, w2_t, u, mask)
    d2, u2 = _rows2d(dy), _rows2d(u)
    M, K = d2.shape
    N = w2_t.shape[0]
    assert dy.dtype == torch.bfloat16 and w2_t.dtype == torch.bfloat16 and u.dtype == torch.bfloat16 and u2.shape == (M, N) and u2.is_contiguous()
    if mask is not None:
        mask = mask.reshape(-1).contiguous()
        assert mask.dtype == torch.bool and mask.numel() == M
    du = torch.empty_like(u)
    _launch(f"gemm_bf16_panel_kernel<{K // 64},gelu_bwd>", 2.0 * M * N * K, 2.0 * (M * K + N * K + 2 * M * N), lib().ispk_gemm_bf16_gelu_bwd,
            d2.data_ptr(), d2.stride(0), w2_t.data_ptr(), w2_t.stride(0), u2.data_ptr(), N, du.data_ptr(), N, _ptr(mask), M, N, K,
            dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _stream())
    return du


def gemm_batched(a: Tensor, w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ispk_gemm_f32_batched: C[i] = a[i] @ w[i]^T for a [batch, M, K], w [batch, N, K] (fp32, unit column strides)
    -> [batch, M, N] (`out`: a view with unit column stride)."""
    _dev(a, w, out)
    assert a.dtype == torch.float32 and w.dtype == torch.float32 and a.ndim == 3 and w.ndim == 3
    assert a.shape[0] == w.shape[0] and a.shape[2] == w.shape[2]
    if a.stride(2) != 1:
        a = a.contiguous()
    if w.stride(2) != 1:
        w = w.contiguous()
    batch, M, K = a.shape
    N = w.shape[1]
    if out is None:
        out = torch.empty((batch, M, N), dtype=torch.float32, device=a.device)
    assert out.shape == (batch, M, N) and out.stride(2) == 1 and out.dtype == torch.float32
    _launch("gemm_f32_kernel<batched>", 2.0 * batch * M * N * K, 4.0 * (a.numel() + w.numel() + out.numel()),
            lib().ispk_gemm_f32_batched, a.data_ptr(), a.stride(1), a.stride(0), w.data_ptr(), w.stride(1), w.stride(0),
            out.data_ptr(), out.stride(1), out.stride(0), batch, M, N, K, _stream())
    return out


def gemm_tn_batched(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ispk_gemm_tn_batched_f32: C[i] = a[i]^T b[i] for a [batch, M, N1], b [batch, M, N2] (fp32; any batch / row strides,
    unit column stride) -> [batch, N1, N2] (`out`: a view with the same freedom)."""
    _dev(a, b, out)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.ndim == 3 and b.ndim == 3 and a.shape[:2] == b.shape[:2]
    if a.stride(2) != 1:
        a = a.contiguous()
    if b.stride(2) != 1:
        b = b.contiguous()
    batch, M, N1 = a.shape
    N2 = b.shape[2]
    if out is None:
        out = torch.empty((batch, N1, N2), dtype=torch.float32, device=a.device)
    assert out.shape == (batch, N1, N2) and out.stride(2) == 1 and out.dtype == torch.float32
    if batch == 0 or M == 0:
        return out if batch == 0 else _zero_rows(out)
    ws = workspace(a.device, batch * N1 * N2)
    _launch("gemm_tn_kernel<batched>", 2.0 * batch * M * N1 * N2, 4.0 * (a.numel() + b.numel() + out.numel()),
            lib().ispk_gemm_tn_batched_f32, a.data_ptr(), a.stride(1), a.stride(0), b.data_ptr(), b.stride(1), b.stride(0),
            out.data_ptr(), out.stride(1), out.stride(0), batch, M, N1, N2, None, 0, ws.data_ptr(), ws.numel(), _stream())
    return out


def aligner_scores_bwd(attn_logits: Tensor, attn_soft: Tensor, d_soft: Optional[Tensor], d_logits: Optional[Tensor],
                       text_len: Tensor, mel_len: Tensor, scale: float):
    """ispk_aligner_scores_bwd_f32 -> (dS [B, M, L4], dSt [B, L, M4]) zero-padded to multiples of 4 columns."""
    _dev(attn_logits, attn_soft, d_soft, d_logits, text_len, mel_len)
    B, M, L = attn_logits.shape
    L4, M4 = (L + 3) // 4 * 4, (M + 3) // 4 * 4
    dS = zeros((B, M, L4), torch.float32, attn_logits.device)
    dSt = zeros((B, L, M4), torch.float32, attn_logits.device)
    cg = lambda t: None if t is None else t.float().contiguous()       # noqa: E731
    d_soft, d_logits = cg(d_soft), cg(d_logits)
    _launch("aligner_scores_bwd_kernel", 0.0, 4.0 * B * M * L * 6, lib().ispk_aligner_scores_bwd_f32, attn_logits.contiguous().data_ptr(),
            attn_soft.contiguous().data_ptr(), _ptr(d_soft), _ptr(d_logits), text_len.to(torch.int64).contiguous().data_ptr(),
            mel_len.to(torch.int64).contiguous().data_ptr(), dS.data_ptr(), L4, dSt.data_ptr(), M4, B, M, L, scale, _stream())
    return dS, dSt


def masked_instnorm_bwd(y: Tensor, d_out: Tensor, weight: Tensor, lengths: Tensor, eps: float = 1e-5):
    """ispk_masked_instnorm_bwd_f32: y, d_out [B, T+4, C] (row t = frame t) -> (d_y like y, d_weight [C], d_bias [C])."""
    _dev(y, d_out, weight, lengths)
    B, TP, C = y.shape
    assert y.is_contiguous() and d_out.is_contiguous() and d_out.shape == y.shape and y.dtype == torch.float32
    d_y = torch.empty_like(y)
    dw, db = torch.empty((C,), dtype=torch.float32, device=y.device), torch.empty((C,), dtype=torch.float32, device=y.device)
    ws = workspace(y.device, 2 * B * C)
    _launch("masked_instnorm_bwd_kernel", 0.0, 4.0 * y.numel() * 5, lib().ispk_masked_instnorm_bwd_f32, y.data_ptr(), d_out.data_ptr(),
            weight.data_ptr(), lengths.to(torch.int64).contiguous().data_ptr(), d_y.data_ptr(), dw.data_ptr(), db.data_ptr(),
            ws.data_ptr(), ws.numel(), B, TP - 4, C, eps, _stream())
    return d_y, dw, db


def soft_average_bwd(attn_soft: Tensor, pitch: Tensor, energy: Tensor, d_feats: Tensor, text_len: Tensor) -> Tensor:
    """ispk_soft_average_bwd_f32 -> d attn_soft [B, M, L]."""
    _dev(attn_soft, pitch, energy, d_feats, text_len)
    B, M, L = attn_soft.shape
    d = torch.empty_like(attn_soft)
    ws = workspace(attn_soft.device, 3 * B * L)
    _launch("soft_average_bwd_kernels", 0.0, 4.0 * attn_soft.numel() * 3, lib().ispk_soft_average_bwd_f32,
            attn_soft.contiguous().data_ptr(), pitch.float().contiguous().data_ptr(), energy.float().contiguous().data_ptr(),
            d_feats.float().contiguous().data_ptr(), text_len.to(torch.int64).contiguous().data_ptr(), ws.data_ptr(), ws.numel(),
            d.data_ptr(), 0, B, M, L, _stream())
    return d


def layernorm_bwd(x: Tensor, dy: Tensor, gamma: Optional[Tensor], row_mask: Optional[Tensor] = None,
                  dx: Optional[Tensor] = None, add_to_dx: bool = False, want_param_grads: bool = True, eps: float = 1e-5,
                  bf16_copy: bool = False):
    """ispk_layernorm_bwd_f32 -> (dx, dgamma | None, dbeta | None).  `dx` given + add_to_dx: accumulated in place (the
    residual branch's gradient is already there).  `bf16_copy` (ispk_layernorm_bwd_dual_f32): a fourth result, dx once more
    as bf16 rows - the operand an AMP step's next dX GEMM and weight gradient take, without a cast launch."""
    _dev(x, dy, gamma, row_mask, dx)
    x2, dy2 = _rows2d(x), _rows2d(dy)
    rows, D = x2.shape
    assert x2.dtype == torch.float32 and dy2.dtype == torch.float32 and dy2.shape == x2.shape
    if dx is None:
        assert not add_to_dx
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dx2 = _rows2d(dx)
    if row_mask is not None:
        row_mask = row_mask.reshape(-1).contiguous()
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    dg = db = None
    ws = None
    if want_param_grads:
        dg = torch.empty((D,), dtype=torch.float32, device=x.device)
        db = torch.empty((D,), dtype=torch.float32, device=x.device)
        ws = workspace(x.device, ((rows + 63) // 64) * 2 * D)
    if bf16_copy:
        dx16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        _launch(f"layernorm_bwd_kernel<{D // 64}>", 0.0, 4.0 * rows * D * (3.5 + int(add_to_dx)), lib().ispk_layernorm_bwd_dual_f32,
                x2.data_ptr(), x2.stride(0), dy2.data_ptr(), dy2.stride(0), _ptr(gamma), _ptr(row_mask), dx2.data_ptr(),
                dx2.stride(0), int(add_to_dx), _ptr(dg), _ptr(db), _ptr(ws), ws.numel() if ws is not None else 0, rows, D, eps,
                dx16.data_ptr(), D, _stream())
        return dx, dg, db, dx16
    _launch(f"layernorm_bwd_kernel<{D // 64}>", 0.0, 4.0 * rows * D * (3 + int(add_to_dx)), lib().ispk_layernorm_bwd_f32,
            x2.data_ptr(), x2.stride(0), dy2.data_ptr(), dy2.stride(0), _ptr(gamma), _ptr(row_mask), dx2.data_ptr(),
            dx2.stride(0), int(add_to_dx), _ptr(dg), _ptr(db), _ptr(ws), ws.numel() if ws is not None else 0, rows, D, eps,
            _stream())
    return dx, dg, db


def gelu(u: Tensor, dropout_p: float = 0.0, seed: int = 0, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_gelu_f32 / ispk_gelu_f32_bf16: exact-erf GELU as its own pass (the training forward keeps u), optionally followed
    by dropout; `out_dtype=torch.bfloat16`: the result as the bf16 operand an AMP step's second Linear takes."""
    _dev(u)
    assert u.dtype in (torch.float32, torch.bfloat16) and u.is_contiguous() and out_dtype in (torch.float32, torch.bfloat16)
    if u.dtype == torch.bfloat16:      # ispk_gelu_bf16: the pre-activation itself is bf16 (autocast's Linear output)
        assert out_dtype == torch.bfloat16
        fn = lib().ispk_gelu_bf16
    else:
        fn = lib().ispk_gelu_f32 if out_dtype == torch.float32 else lib().ispk_gelu_f32_bf16
    a = torch.empty(u.shape, dtype=out_dtype, device=u.device)
    _launch("gelu_fwd_kernel", 0.0, float(u.element_size() + a.element_size()) * u.numel(), fn, u.data_ptr(), a.data_ptr(), u.numel(),
            dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _stream())
    return a


def dropout_mask(n: int, dropout_p: float, seed: int, device) -> Tensor:
    """ispk_dropout_mask_u8: the keep mask the kernels evaluate for element indices 0 .. n-1 (bool [n])."""
    out = torch.empty((n,), dtype=torch.bool, device=device)
    _dev(out)
    _check(lib().ispk_dropout_mask_u8(out.data_ptr(), n, dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _stream()), "ispk_dropout_mask_u8")
    return out


def alibi_mqa_attention_train(qkv: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor], dropout_p: float, seed: int):
    """-> (o [B, N, heads*64] in qkv's dtype, lse fp32 [B, heads, N]): attention with dropped probabilities, row statistics
    kept for the backward.  fp32 qkv: ispk_alibi_mqa_attn_train_f32.  bf16 qkv (the step under autocast):
    ispk_alibi_mqa_attn_train_bf16 - bf16 MFMAs, K / V staged in LDS, bf16 o."""
    _dev(qkv, slopes, key_len)
    B, N, W = qkv.shape
    b16 = qkv.dtype == torch.bfloat16
    assert W == heads * 64 + 128 and qkv.dtype in (torch.float32, torch.bfloat16) and qkv.is_contiguous()
    slopes = slopes.to(torch.float32).contiguous()
    if key_len is not None:
        key_len = key_len.to(torch.int64).contiguous()
    o = torch.empty((B, N, heads * 64), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see alibi_mqa_attention_raw)
        return o, lse
    _launch("attn_train_fwd_bf16_kernel" if b16 else "attn_train_fwd_kernel", 4.0 * B * heads * N * N * 64,
            float(qkv.element_size()) * (qkv.numel() + o.numel()),
            lib().ispk_alibi_mqa_attn_train_bf16 if b16 else lib().ispk_alibi_mqa_attn_train_f32, qkv.data_ptr(), W, slopes.data_ptr(),
            _ptr(key_len), o.data_ptr(), heads * 64, lse.data_ptr(), B, N, heads, dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _stream())
    return o, lse


def gelu_bwd(da: Tensor, u: Tensor, out: Optional[Tensor] = None, dropout_p: float = 0.0, seed: int = 0) -> Tensor:
    """ispk_gelu_bwd_f32: du = da * [keep / (1 - p)] * gelu'(u) (exact erf); `out` may alias `da`."""
    _dev(da, u, out)
    assert da.dtype in (torch.float32, torch.bfloat16) and u.dtype in (torch.float32, torch.bfloat16) and da.is_contiguous() and u.is_contiguous()
    assert da.shape == u.shape and (u.dtype == torch.float32 or da.dtype == torch.bfloat16)
    if out is None:
        out = torch.empty_like(da)
    assert out.dtype == da.dtype
    b16 = da.dtype == torch.bfloat16      # ispk_gelu_bwd_bf16: da and du are bf16 GEMM operands of an AMP step (_b16: u bf16 too)
    fn = (lib().ispk_gelu_bwd_b16 if u.dtype == torch.bfloat16 else lib().ispk_gelu_bwd_bf16) if b16 else lib().ispk_gelu_bwd_f32
    _launch("gelu_bwd_kernel", 0.0, float(u.element_size() + 2 * da.element_size()) * da.numel(), fn,
            da.data_ptr(), u.data_ptr(), out.data_ptr(), da.numel(), dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _stream())
    return out


def alibi_mqa_attention_bwd(qkv: Tensor, o: Tensor, d_o: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor],
                            lse: Optional[Tensor] = None, dropout_p: float = 0.0, seed: int = 0):
    """-> (dqkv like qkv, dlogslopes fp32 [heads]).  fp32 tensors: ispk_alibi_mqa_attn_bwd_f32 (`lse` from the training
    forward saves the statistics pass).  bf16 tensors (the step under autocast): ispk_alibi_mqa_attn_bwd_bf16, `lse` required.
    dropout_p / seed must be the forward's."""
    _dev(qkv, o, d_o, slopes, key_len, lse)
    B, N, W = qkv.shape
    b16 = qkv.dtype == torch.bfloat16
    assert W == heads * 64 + 128 and qkv.dtype in (torch.float32, torch.bfloat16) and qkv.is_contiguous()
    assert o.shape == (B, N, heads * 64) and d_o.shape == o.shape and o.dtype == qkv.dtype and d_o.dtype == qkv.dtype
    o, d_o = o.contiguous(), d_o.contiguous()
    slopes = slopes.to(torch.float32).contiguous()
    if key_len is not None:
        key_len = key_len.to(torch.int64).contiguous()
    dqkv = torch.empty_like(qkv)
    dls = torch.empty((heads,), dtype=torch.float32, device=qkv.device)
    if B == 0:      # no rows, no gradient (NULL data_ptr() of an empty tensor: see alibi_mqa_attention_raw)
        return dqkv, dls.zero_()
    if b16:
        assert lse is not None and lse.dtype == torch.float32 and lse.shape == (B, heads, N) and lse.is_contiguous()
        ws = workspace(qkv.device, B * heads * N + 2 * heads * B * ((N + 63) // 64))
        _launch("attn_bwd_bf16_kernels", 10.0 * B * heads * N * N * 64, 2.0 * (2 * qkv.numel() + 2 * o.numel()),
                lib().ispk_alibi_mqa_attn_bwd_bf16, qkv.data_ptr(), W, o.data_ptr(), d_o.data_ptr(), heads * 64, slopes.data_ptr(),
                _ptr(key_len), lse.data_ptr(), dqkv.data_ptr(), dls.data_ptr(), ws.data_ptr(), ws.numel(), B, N, heads, dropout_p,
                seed & 0xFFFFFFFFFFFFFFFF, _stream())
        return dqkv, dls
    tiles = (N + 31) // 32
    ws = workspace(qkv.device, 2 * B * heads * N + heads * B * tiles)
    _launch("attn_bwd_kernels", 10.0 * B * heads * N * N * 64, 4.0 * (2 * qkv.numel() + 2 * o.numel()),
            lib().ispk_alibi_mqa_attn_bwd_f32, qkv.data_ptr(), W, o.data_ptr(), d_o.data_ptr(), heads * 64, slopes.data_ptr(),
            _ptr(key_len), dqkv.data_ptr(), dls.data_ptr(), ws.data_ptr(), ws.numel(), B, N, heads, _ptr(lse), dropout_p,
            seed & 0xFFFFFFFFFFFFFFFF, _stream())
    return dqkv, dls


def mel_loss(mel_out: Tensor, mel_target: Tensor, mel_len: Tensor, want_grad: bool = False, grad_out: float = 1.0):
    """ispk_mel_loss_f32 -> (loss fp32 [1], grad fp32 like mel_out | None)."""
    _dev(mel_out, mel_target, mel_len)
    assert mel_out.dtype == torch.float32 and mel_target.dtype == torch.float32 and mel_out.shape == mel_target.shape
    mel_out, mel_target = mel_out.contiguous(), mel_target.contiguous()
    B, C, T = mel_out.shape
    mel_len = mel_len.to(torch.int64).contiguous()
    ratio = torch.empty((B,), dtype=torch.float32, device=mel_out.device)
    loss = torch.empty((1,), dtype=torch.float32, device=mel_out.device)
    grad = torch.empty_like(mel_out) if want_grad else None
    _launch("mel_loss_kernel", 0.0, 4.0 * mel_out.numel() * (2 + int(want_grad)), lib().ispk_mel_loss_f32, mel_out.data_ptr(),
            mel_target.data_ptr(), mel_len.data_ptr(), ratio.data_ptr(), loss.data_ptr(), _ptr(grad), grad_out, B, C, T,
            _stream())
    return loss, grad


METRICS_CHUNK = 32     # frames per workgroup of ispk_acoustic_metrics_f32 (its workspace: 3 partials per item and chunk)


def metrics_workspace_floats(B: int, T: int) -> int:
    return 3 * B * ((T + METRICS_CHUNK - 1) // METRICS_CHUNK)


def _mel_strides(x: Tensor, C: int):
    """(C', T, sb, sc, st) of a mel as MCD._mfcc (evaluator.py:28-31) reads it: [B, T, C] when size(-1) == C, else
    [B, C, T] (so a [B, C, C] mel is read frames-first: the axes are swapped)."""
    if x.shape[-1] == C:
        return x.shape[2], x.shape[1], x.stride(0), x.stride(2), x.stride(1)
    return x.shape[1], x.shape[2], x.stride(0), x.stride(1), x.stride(2)


def acoustic_metrics(mel_out: Optional[Tensor], mel_target: Optional[Tensor], mel_len: Tensor, text_len: Optional[Tensor],
                     attn_soft: Optional[Tensor], dct: Optional[Tensor], out: Optional[Tensor] = None) -> Tensor:
    """ispk_acoustic_metrics_f32 -> fp32 [3] on the device = (mcd, alignment_length, alignment_strength), no host read.
    mel_out / mel_target fp32 [B, C, T] or [B, T, C] (any strides; C = dct.shape[0], the layout rule of MCD._mfcc), dct fp32
    [C, n_mfcc] on the device, attn_soft fp32 [B, T, L] (unit stride on L), lengths int64 [B].  Either the mels (with dct)
    or attn_soft (with text_len) may be None: that part of `out` is then not written.  B = 0 gives NaN for all three
    without a launch, as the reference's means over an empty batch (0 / 0)."""
    _dev(mel_out, mel_target, mel_len, text_len, attn_soft, dct, out)
    if out is None:
        out = torch.empty((3,), dtype=torch.float32, device=mel_len.device)
    assert out.dtype == torch.float32 and out.numel() == 3 and out.is_contiguous()
    B = mel_len.shape[0]
    if B == 0:
        return out.fill_(float("nan"))
    mel_len = mel_len.to(torch.int64).contiguous()
    C = n_mfcc = T = L = 0
    m = mt = (0,) * 5                   # (strides of an absent mel pair: not read)
    if mel_out is not None or mel_target is not None:
        assert mel_out is not None and mel_target is not None and dct is not None
        assert mel_out.dtype == torch.float32 and mel_target.dtype == torch.float32 and dct.dtype == torch.float32
        assert mel_out.ndim == 3 and mel_target.ndim == 3 and dct.ndim == 2 and dct.is_contiguous()
        C, n_mfcc = dct.shape
        m, mt = _mel_strides(mel_out, C), _mel_strides(mel_target, C)
        if m[0] != C or mt[0] != C or m[1] != mt[1] or mel_out.shape[0] != B or mel_target.shape[0] != B:
            raise ValueError(f"mels {tuple(mel_out.shape)} / {tuple(mel_target.shape)} do not match {C} channels and {B} lengths")
        T = m[1]
    if attn_soft is not None:
        assert attn_soft.dtype == torch.float32 and attn_soft.ndim == 3 and text_len is not None
        if attn_soft.stride(2) != 1:
            attn_soft = attn_soft.contiguous()
        if attn_soft.shape[0] != B or (T and attn_soft.shape[1] != T):
            raise ValueError(f"attention {tuple(attn_soft.shape)} does not match {B} items of {T} frames")
        T, L = attn_soft.shape[1], attn_soft.shape[2]
        text_len = text_len.to(torch.int64).contiguous()
    ws = torch.empty((metrics_workspace_floats(B, T),), dtype=torch.float32, device=mel_len.device)
    nbytes = 4.0 * (2 * B * C * T + (attn_soft.numel() if attn_soft is not None else 0))
    _launch("acoustic_metrics_kernels", 2.0 * B * T * C * n_mfcc, nbytes, lib().ispk_acoustic_metrics_f32,
            _ptr(mel_out), m[2], m[3], m[4], _ptr(mel_target), mt[2], mt[3], mt[4], mel_len.data_ptr(),
            _ptr(text_len) if attn_soft is not None else None, _ptr(attn_soft),
            attn_soft.stride(0) if attn_soft is not None else 0, attn_soft.stride(1) if attn_soft is not None else 0,
            _ptr(dct), ws.data_ptr(), ws.numel(), out.data_ptr(), B, C, T, L, n_mfcc, _stream())
    return out


DTW_MAX_LEN = 2048     # frames per side of ispk_dtw_f32 / ispk_mcd_dtw_f32
DTW_LANES = 256        # lanes per item; each owns 1, 2, 4 or 8 rows


def dtw_workspace_floats(B: int, N: int, M: int) -> int:
    """ispk_dtw_f32: per item the skewed copy of the costs ((M + 255) rows of 256 R floats: a row is one step of a wave) and the
    2-bit back-pointers (per lane, words of 16 / R columns x R rows)."""
    R = 1 if N <= 256 else (2 if N <= 512 else (4 if N <= 1024 else 8))
    return B * DTW_LANES * ((M + DTW_LANES - 1) * R + (M * R + 15) // 16)


def mcd_dtw_workspace_floats(B: int, N: int, M: int, n_mfcc: int) -> int:
    """ispk_mcd_dtw_f32: ispk_dtw_f32's, the cepstra of both mels, totals and steps."""
    kp = (n_mfcc - 1 + 3) // 4 * 4
    return dtw_workspace_floats(B, N, M) + B * (N + M) * kp + 2 * B


def dtw(cost: Tensor, n_len: Tensor, m_len: Tensor, want_path: bool = True):
    """ispk_dtw_f32.  cost fp32 [B, N, M] (unit stride on M), lengths int64 [B] on the device -> (total fp32 [B], steps int32
    [B], path int16 [B, N + M - 1, 2] | None): the cells of the warping path from (0, 0), -1 past `steps`.  No host read."""
    _dev(cost, n_len, m_len)
    assert cost.dtype == torch.float32 and cost.ndim == 3
    if cost.stride(2) != 1:
        cost = cost.contiguous()
    B, N, M = cost.shape
    n_len, m_len = n_len.to(torch.int64).contiguous(), m_len.to(torch.int64).contiguous()
    assert n_len.shape == (B,) and m_len.shape == (B,)
    total = torch.empty((B,), dtype=torch.float32, device=cost.device)
    steps = torch.empty((B,), dtype=torch.int32, device=cost.device)
    path = torch.empty((B, N + M - 1, 2), dtype=torch.int16, device=cost.device) if want_path else None
    if B == 0:
        return total, steps, path
    ws = workspace(cost.device, dtw_workspace_floats(B, N, M))
    _launch("dtw_kernel", 4.0 * B * N * M, 12.25 * B * N * M, lib().ispk_dtw_f32, cost.data_ptr(), cost.stride(0), cost.stride(1),
            n_len.data_ptr(), m_len.data_ptr(), total.data_ptr(), steps.data_ptr(), _ptr(path), ws.data_ptr(), ws.numel(), B, N,
            M, _stream())
    return total, steps, path


def mcd_dtw(mel_out: Tensor, mel_out_len: Tensor, mel_target: Tensor, mel_target_len: Tensor, dct: Tensor,
            pitch_out: Optional[Tensor] = None, pitch_target: Optional[Tensor] = None, out: Optional[Tensor] = None,
            cost_out: Optional[Tensor] = None):
    """ispk_mcd_dtw_f32 -> (per_item fp32 [4, B], means fp32 [4]), two views of ONE device buffer of 4 B + 4 floats (`out`,
    when given): rows / elements 0 .. 3 are (mcd_dtw, f0_rmse_cents, vuv_error, length_ratio).  mels fp32 [B, C, T] or
    [B, T, C] under the layout rule of `_mel_strides`, dct fp32 [C, n_mfcc] on the device, lengths int64 [B], pitch fp32
    [B, >= T] in Hz with 0 = unvoiced (both or neither: without them rows 1 and 2 are not written).  `cost_out`: fp32 [B, N, M]
    (contiguous) that receives each item's n_len x m_len costs.  No host read.  B = 0 gives NaN means without a launch."""
    _dev(mel_out, mel_out_len, mel_target, mel_target_len, dct, pitch_out, pitch_target, out, cost_out)
    assert mel_out.dtype == torch.float32 and mel_target.dtype == torch.float32 and dct.dtype == torch.float32
    assert mel_out.ndim == 3 and mel_target.ndim == 3 and dct.ndim == 2 and dct.is_contiguous()
    assert (pitch_out is None) == (pitch_target is None)
    B = mel_out_len.shape[0]
    C, n_mfcc = dct.shape
    m, mt = _mel_strides(mel_out, C), _mel_strides(mel_target, C)
    if m[0] != C or mt[0] != C or mel_out.shape[0] != B or mel_target.shape[0] != B or mel_target_len.shape[0] != B:
        raise ValueError(f"mels {tuple(mel_out.shape)} / {tuple(mel_target.shape)} do not match {C} channels and {B} lengths")
    N, M = m[1], mt[1]
    if out is None:
        out = torch.empty((4 * B + 4,), dtype=torch.float32, device=mel_out.device)
    assert out.dtype == torch.float32 and out.shape == (4 * B + 4,) and out.is_contiguous()
    per_item, means = out[:4 * B].view(4, B), out[4 * B:]
    if B == 0:
        out.fill_(float("nan"))
        return per_item, means
    n_len, m_len = mel_out_len.to(torch.int64).contiguous(), mel_target_len.to(torch.int64).contiguous()
    if pitch_out is not None:
        assert pitch_out.dtype == torch.float32 and pitch_target.dtype == torch.float32
        assert pitch_out.ndim == 2 and pitch_target.ndim == 2 and pitch_out.shape[0] == B and pitch_target.shape[0] == B
        if pitch_out.shape[1] < N or pitch_target.shape[1] < M:
            raise ValueError(f"pitch tracks {tuple(pitch_out.shape)} / {tuple(pitch_target.shape)} are shorter than the mels")
        if pitch_out.stride(1) != 1:
            pitch_out = pitch_out.contiguous()
        if pitch_target.stride(1) != 1:
            pitch_target = pitch_target.contiguous()
    ws = workspace(mel_out.device, mcd_dtw_workspace_floats(B, N, M, n_mfcc))
    if cost_out is not None:
        assert cost_out.dtype == torch.float32 and cost_out.shape == (B, N, M) and cost_out.is_contiguous()
    _launch("mcd_dtw_kernels", 2.0 * B * (N + M) * C * n_mfcc + 3.0 * B * N * M * n_mfcc, 8.25 * B * N * M,
            lib().ispk_mcd_dtw_f32, mel_out.data_ptr(), m[2], m[3], m[4], mel_target.data_ptr(), mt[2], mt[3], mt[4],
            dct.data_ptr(), n_len.data_ptr(), m_len.data_ptr(), _ptr(pitch_out),
            pitch_out.stride(0) if pitch_out is not None else 0, _ptr(pitch_target),
            pitch_target.stride(0) if pitch_target is not None else 0, ws.data_ptr(), ws.numel(), per_item.data_ptr(),
            means.data_ptr(), _ptr(cost_out), B, C, N, M, n_mfcc, _stream())
    return per_item, means


FEATURE_HOP = 256          # STFT / YIN hop of ispk_audio_features_f32 (n_fft = win_length = 1024, pad 384 on each side)
FEATURE_TABLE_HEAD = 5120  # tables[0, 5120): W_2048^m as (re, im), then the Hann window; the filterbank weights follow


def feature_frames(samples: int) -> int:
    """Frames of an utterance of `samples` samples: (S + 768 - 1024) // 256 + 1, 0 below 256 samples (where torch.stft raises)."""
    return (samples - FEATURE_HOP) // FEATURE_HOP + 1 if samples >= FEATURE_HOP else 0


def audio_features(audio: Tensor, audio_len: Tensor, tables: Tensor, fb_index: Optional[Tensor], mel: Optional[Tensor],
                   mel_len: Optional[Tensor], pitch: Optional[Tensor], energy: Optional[Tensor], tau_min: int = 1,
                   tau_max: int = 512, sample_rate: float = 0.0, threshold: float = 0.0, pitch_mean: float = 0.0,
                   pitch_std: float = 1.0) -> None:
    """ispk_audio_features_f32, one launch, no host read: fills the given outputs (each may be None) of the fp32 waveforms
    audio [B, S] (unit stride on S, any row stride) with int64 lengths audio_len [B].  mel fp32 [B, n_mels, M], pitch / energy
    fp32 [B, M], mel_len int64 [B], all contiguous; tables fp32 and fb_index int32 as include/ispk.h lays them out
    (data.AcousticFeatures builds them).  The kernel reads no filterbank weight past tables.numel(), whatever fb_index
    (device data, not read here) says."""
    _dev(audio, audio_len, tables, fb_index, mel, mel_len, pitch, energy)
    assert audio.dtype == torch.float32 and audio.ndim == 2 and audio.stride(1) == 1, "audio: fp32 [B, S], unit stride on S"
    assert audio_len.dtype == torch.int64 and audio_len.ndim == 1 and audio_len.is_contiguous()
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= FEATURE_TABLE_HEAD
    B, S = audio.shape
    if audio_len.shape[0] != B:
        raise ValueError(f"{audio_len.shape[0]} lengths for {B} waveforms")
    M, n_mels = None, 0
    for name, t, dt, nd in (("mel", mel, torch.float32, 3), ("pitch", pitch, torch.float32, 2),
                            ("energy", energy, torch.float32, 2), ("mel_len", mel_len, torch.int64, 1)):
        if t is None:
            continue
        if t.dtype != dt or t.ndim != nd or not t.is_contiguous() or t.shape[0] != B:
            raise ValueError(f"{name}: need a contiguous {dt} tensor of {nd} dims and {B} rows, got {t.dtype} {tuple(t.shape)}")
        if nd > 1:
            if M is not None and t.shape[-1] != M:
                raise ValueError(f"{name}: {t.shape[-1]} frames, another output has {M}")
            M = t.shape[-1]
    if mel is not None:
        n_mels = mel.shape[1]
        assert fb_index is not None and fb_index.dtype == torch.int32 and fb_index.numel() == 2 * n_mels + 1
    if B == 0:
        return
    _launch("features_kernel", 0.0, 4.0 * audio.numel() + 4.0 * (n_mels + 2) * B * (M or 0), lib().ispk_audio_features_f32,
            audio.data_ptr(), audio.stride(0), audio_len.data_ptr(), tables.data_ptr(), tables.numel(), _ptr(fb_index), n_mels, _ptr(mel),
            _ptr(mel_len), _ptr(pitch), _ptr(energy), B, S, M if M is not None else feature_frames(S), tau_min, tau_max,
            sample_rate, threshold, pitch_mean, pitch_std, _stream())


def resampled_samples(samples: int, orig: int, dest: int) -> int:
    """ceil(dest * samples / orig): the output length of `samples` input samples at the reduced rates orig -> dest."""
    return (samples * dest + orig - 1) // orig


def resample(audio: Tensor, audio_len: Tensor, taps: Tensor, first: Tensor, orig: int, dest: int, width: int,
             out: Optional[Tensor] = None, out_len: Optional[Tensor] = None):
    """ispk_resample_f32, one launch, no host read: fp32 audio [B, S] or [B, C, S] (unit stride on S) with int64 lengths
    [B] -> (fp32 [B, ceil(dest S / orig)], int64 [B]); several channels are averaged.  `orig`, `dest` are the reduced rates,
    taps fp32 [dest, T] / first int32 [dest] the compact polyphase table (data.Resampler builds it)."""
    _dev(audio, audio_len, taps, first, out, out_len)
    if audio.dtype != torch.float32 or audio.ndim not in (2, 3) or audio.stride(-1) != 1:
        raise ValueError(f"audio: fp32 [B, S] or [B, C, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} "
                         f"strides {tuple(audio.stride())}")
    B, S = audio.shape[0], audio.shape[-1]
    C = audio.shape[1] if audio.ndim == 3 else 1
    if audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous():
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    assert taps.dtype == torch.float32 and taps.ndim == 2 and taps.is_contiguous() and taps.shape[0] == dest
    assert first.dtype == torch.int32 and first.shape == (dest,) and first.is_contiguous()
    S_out = resampled_samples(S, orig, dest)
    if out is None:
        out = torch.empty((B, S_out), dtype=torch.float32, device=audio.device)
    if out_len is None:
        out_len = torch.empty((B,), dtype=torch.int64, device=audio.device)
    if out.dtype != torch.float32 or out.shape != (B, S_out) or out.stride(1) != 1:
        raise ValueError(f"out: fp32 [{B}, {S_out}] with unit stride on the samples, got {out.dtype} {tuple(out.shape)}")
    if out_len.dtype != torch.int64 or out_len.shape != (B,) or not out_len.is_contiguous():
        raise ValueError(f"out_len: contiguous int64 [{B}], got {out_len.dtype} {tuple(out_len.shape)}")
    if B == 0:
        return out, out_len
    _launch("resample_kernel", 2.0 * taps.shape[1] * B * S_out, 4.0 * (B * C * S + B * S_out), lib().ispk_resample_f32,
            audio.data_ptr(), audio.stride(0), audio.stride(1) if audio.ndim == 3 else 0, audio_len.data_ptr(),
            taps.data_ptr(), taps.numel(), first.data_ptr(), out.data_ptr(), out.stride(0), out_len.data_ptr(), B, C, S, S_out,
            orig, dest, width, taps.shape[1], _stream())
    return out, out_len


STATS_MAX_FRAMES = 4096    # ispk_feature_stats_f64 sorts an utterance in LDS


def feature_stats(pitch: Optional[Tensor], energy: Optional[Tensor], mel_len: Optional[Tensor], partial: Optional[Tensor],
                  state: Tensor, reset: bool = False) -> None:
    """ispk_feature_stats_f64, a launch pair, no host read: the per-utterance outlier-filtered (count, mean, M2, min, max) of
    pitch / energy fp32 [B, M] into partial float64 [B, 2, 5], folded in utterance order into state float64 [2, 5].  With
    pitch None (and reset) it only writes the empty state."""
    _dev(pitch, energy, mel_len, partial, state)
    assert state.dtype == torch.float64 and state.shape == (2, 5) and state.is_contiguous()
    if pitch is None:
        _launch("stats_fold_kernel", 0.0, 80.0, lib().ispk_feature_stats_f64, None, 0, None, 0, None, None, state.data_ptr(),
                0, 0, int(reset), _stream())
        return
    for name, t in (("pitch", pitch), ("energy", energy)):
        if t.dtype != torch.float32 or t.ndim != 2 or t.stride(1) != 1 or t.shape != pitch.shape:
            raise ValueError(f"{name}: fp32 {tuple(pitch.shape)} with unit stride on the frames, got {t.dtype} {tuple(t.shape)} "
                             f"strides {tuple(t.stride())}")
    B, M = pitch.shape
    if mel_len.dtype != torch.int64 or mel_len.shape != (B,) or not mel_len.is_contiguous():
        raise ValueError(f"mel_len: contiguous int64 [{B}], got {mel_len.dtype} {tuple(mel_len.shape)}")
    assert partial.dtype == torch.float64 and partial.shape == (B, 2, 5) and partial.is_contiguous()
    _launch("feature_stats_kernel", 0.0, 8.0 * B * M, lib().ispk_feature_stats_f64, pitch.data_ptr(), pitch.stride(0),
            energy.data_ptr(), energy.stride(0), mel_len.data_ptr(), partial.data_ptr(), state.data_ptr(), B, M, int(reset),
            _stream())


CONDITION_TABLE_DOUBLES = 152     # 7 coefficients, one unused, nine 4 x 4 powers of the state transition (include/ispk.h)
CONDITION_MAX_SAMPLES = 1 << 24
CONDITION_RATES = (8000, 768000)


def audio_measure_workspace_floats(B: int, S: int, sample_rate: int) -> int:
    """ispk_audio_measure_f64: per item the 256-sample square sums, the final states of every 32-sample chunk (4 doubles) and
    8,192-sample segment, 12 step partials and a peak per segment, and the step sums - in doubles, two floats each."""
    W, NH, NS = max(1, -(-S // 8192)), max(1, -(-S // 256)), S // (sample_rate // 10) + 1
    return 2 * B * (NH + W * (256 * 4 + 4 + 12 + 1) + NS)


def _mono_batch(audio: Tensor, audio_len: Optional[Tensor]) -> tuple[int, int]:
    if audio.dtype != torch.float32 or audio.ndim != 2 or audio.stride(1) != 1:
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    B, S = audio.shape
    if S > CONDITION_MAX_SAMPLES or B > 65535:
        raise ValueError(f"audio: at most 65535 utterances of {CONDITION_MAX_SAMPLES} samples, got {tuple(audio.shape)}")
    if audio_len is not None and (audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous()):
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    return B, S


def _out_like(name: str, t: Tensor, dtype, shape) -> None:
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or (t.ndim and t.stride(-1) != 1) or (t.ndim == 1 and not t.is_contiguous()):
        raise ValueError(f"{name}: {dtype} {tuple(shape)} with unit stride on the last axis, got {t.dtype} {tuple(t.shape)}")


def audio_measure(audio: Tensor, audio_len: Tensor, table: Tensor, sample_rate: int, trim_mode: int, trim_threshold: float,
                  pad_frames: int, gain_mode: int, target_lufs: float, peak_limit: float, bounds: Optional[Tensor] = None,
                  loudness: Optional[Tensor] = None, peak: Optional[Tensor] = None, gain: Optional[Tensor] = None):
    """ispk_audio_measure_f64, three launches, no host read: fp32 audio [B, S] (unit stride on S) with int64 lengths [B] ->
    (bounds int64 [B, 2], loudness float64 [B], peak fp32 [B], gain fp32 [B]).  `table` float64 [152] as include/ispk.h lays
    it out (data.AudioConditioner builds it)."""
    _dev(audio, audio_len, table, bounds, loudness, peak, gain)
    B, S = _mono_batch(audio, audio_len)
    assert table.dtype == torch.float64 and table.shape == (CONDITION_TABLE_DOUBLES,) and table.is_contiguous()
    dev = audio.device
    bounds = torch.empty((B, 2), dtype=torch.int64, device=dev) if bounds is None else bounds
    loudness = torch.empty((B,), dtype=torch.float64, device=dev) if loudness is None else loudness
    peak = torch.empty((B,), dtype=torch.float32, device=dev) if peak is None else peak
    gain = torch.empty((B,), dtype=torch.float32, device=dev) if gain is None else gain
    _out_like("bounds", bounds, torch.int64, (B, 2))
    if not bounds.is_contiguous():
        raise ValueError("bounds: contiguous int64 [B, 2]")
    _out_like("loudness", loudness, torch.float64, (B,))
    _out_like("peak", peak, torch.float32, (B,))
    _out_like("gain", gain, torch.float32, (B,))
    if B == 0:
        return bounds, loudness, peak, gain
    ws = workspace(dev, audio_measure_workspace_floats(B, S, sample_rate))
    _launch("audio_measure_kernels", 56.0 * B * S, 4.0 * 2 * B * S + 2.0 * 8 * B * S / 8, lib().ispk_audio_measure_f64, audio.data_ptr(),
            audio.stride(0), audio_len.data_ptr(), table.data_ptr(), table.numel(), bounds.data_ptr(), loudness.data_ptr(),
            peak.data_ptr(), gain.data_ptr(), ws.data_ptr(), ws.numel(), B, S, int(sample_rate), int(trim_mode),
            float(trim_threshold), int(pad_frames), int(gain_mode), float(target_lufs), float(peak_limit), _stream())
    return bounds, loudness, peak, gain


def audio_apply(audio: Tensor, bounds: Tensor, gain: Optional[Tensor], out: Optional[Tensor] = None,
                out_len: Optional[Tensor] = None):
    """ispk_audio_apply_f32, one launch: out[b, i] = gain[b] * audio[b, start_b + i] below end_b - start_b, then zeros; the
    lengths go to out_len.  `out` fp32 [B, S_out] may not overlap `audio`."""
    _dev(audio, bounds, gain, out, out_len)
    B, S = _mono_batch(audio, None)
    dev = audio.device
    out = torch.empty((B, S), dtype=torch.float32, device=dev) if out is None else out
    out_len = torch.empty((B,), dtype=torch.int64, device=dev) if out_len is None else out_len
    if out.ndim != 2:
        raise ValueError(f"out: fp32 [{B}, S_out], got {tuple(out.shape)}")
    _out_like("out", out, torch.float32, (B, out.shape[1]))
    _out_like("out_len", out_len, torch.int64, (B,))
    _out_like("bounds", bounds, torch.int64, (B, 2))
    if gain is not None:
        _out_like("gain", gain, torch.float32, (B,))
    if B == 0:
        return out, out_len
    _launch("cond_apply_kernel", 1.0 * B * S, 4.0 * (B * S + out.numel()), lib().ispk_audio_apply_f32, audio.data_ptr(), audio.stride(0),
            bounds.data_ptr(), _ptr(gain), out.data_ptr(), out.stride(0), out_len.data_ptr(), B, S, out.shape[1], _stream())
    return out, out_len


def pcm16(audio: Tensor, audio_len: Tensor, dither: bool = False, seed: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """ispk_pcm16, one launch: fp32 [B, S] -> int16 [B, S], clamp(rint(32768 x + d)), zero past audio_len."""
    _dev(audio, audio_len, out)
    B, S = _mono_batch(audio, audio_len)
    out = torch.empty((B, S), dtype=torch.int16, device=audio.device) if out is None else out
    _out_like("out", out, torch.int16, (B, S))
    if B == 0 or S == 0:
        return out
    _launch("pcm16_kernel", 0.0, 6.0 * B * S, lib().ispk_pcm16, audio.data_ptr(), audio.stride(0), audio_len.data_ptr(),
            out.data_ptr(), out.stride(0), B, S, int(bool(dither)), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream())
    return out


def flow_loss_bwd(pred_raw: Tensor, flow: Tensor, mask: Tensor, grad_out: float = 1.0) -> Tensor:
    """ispk_flow_loss_bwd_f32: gradient of the flow loss wrt the predictor's raw output [B, L, C]."""
    _dev(pred_raw, flow, mask)
    pred_raw, flow, mask = pred_raw.contiguous(), flow.contiguous(), mask.contiguous()
    B, L, C = pred_raw.shape
    assert mask.dtype == torch.bool and mask.shape == (B, L) and flow.shape == pred_raw.shape
    d = torch.empty_like(pred_raw)
    _launch("flow_loss_bwd_kernel", 0.0, 12.0 * pred_raw.numel(), lib().ispk_flow_loss_bwd_f32, pred_raw.data_ptr(), flow.data_ptr(),
            mask.data_ptr(), grad_out, d.data_ptr(), B, L, C, _stream())
    return d


def adaln_bwd(x: Tensor, dy: Tensor, scale: Tensor, row_mask: Optional[Tensor], dx: Optional[Tensor], add_to_dx: bool,
              dscale: Tensor, dshift: Tensor, eps: float = 1e-5) -> Tensor:
    """ispk_adaln_bwd_f32: x, dy [B, L, D]; scale / dscale / dshift [B, D] rows (any row stride, unit column stride)."""
    _dev(x, dy, scale, row_mask, dx, dscale, dshift)
    B, L, D = x.shape
    x2, dy2 = _rows2d(x), _rows2d(dy)
    if dx is None:
        assert not add_to_dx
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dx2 = _rows2d(dx)
    if row_mask is not None:
        row_mask = row_mask.reshape(-1).contiguous()
    assert scale.stride(1) == 1 and dscale.stride(1) == 1 and dshift.stride(1) == 1 and dscale.stride(0) == dshift.stride(0)
    _launch(f"adaln_bwd_kernel<{D // 64}>", 0.0, 4.0 * x2.numel() * (3 + int(add_to_dx)), lib().ispk_adaln_bwd_f32, x2.data_ptr(),
            x2.stride(0), dy2.data_ptr(), dy2.stride(0), scale.data_ptr(), scale.stride(0), _ptr(row_mask), dx2.data_ptr(),
            dx2.stride(0), int(add_to_dx), dscale.data_ptr(), dshift.data_ptr(), dscale.stride(0), B, L, D, eps, _stream())
    return dx


def time_embedding_bwd(t: Tensor, inv_freq: Tensor, freq_scale: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, d_out: Tensor):
    """ispk_time_embedding_bwd_f32 -> (dw0, db0, dw1, db1)."""
    _dev(t, inv_freq, freq_scale, w0, b0, w1, d_out)
    t = t.reshape(-1).float().contiguous()
    d_out = d_out.reshape(t.numel(), -1).float().contiguous()
    E, H = w1.shape[0], inv_freq.numel()
    dw0, db0 = torch.empty_like(w0, dtype=torch.float32), torch.empty((E,), dtype=torch.float32, device=t.device)
    dw1, db1 = torch.empty((E, E), dtype=torch.float32, device=t.device), torch.empty((E,), dtype=torch.float32, device=t.device)
    _launch("time_embedding_bwd_kernel", 0.0, 0.0, lib().ispk_time_embedding_bwd_f32, t.data_ptr(), t.numel(),
            inv_freq.contiguous().data_ptr(), freq_scale.data_ptr(), H, w0.contiguous().data_ptr(), b0.data_ptr(),
            w1.contiguous().data_ptr(), E, d_out.data_ptr(), dw0.data_ptr(), db0.data_ptr(), dw1.data_ptr(), db1.data_ptr(), _stream())
    return dw0, db0, dw1, db1


def attn_ctc_loss(attn_logits: Tensor, text_len: Tensor, mel_len: Tensor, blank_logprob: float = -1.0,
                  want_grad: bool = False, grad_out: float = 1.0):
    """ispk_attn_ctc_loss_f32 -> (loss fp32 [1], grad fp32 like attn_logits | None)."""
    _dev(attn_logits, text_len, mel_len)
    assert attn_logits.dtype == torch.float32
    lg = attn_logits.reshape(-1, *attn_logits.shape[-2:]).contiguous()
    B, M, L = lg.shape
    text_len, mel_len = text_len.to(torch.int64).contiguous(), mel_len.to(torch.int64).contiguous()
    s_pad = (2 * L + 1 + 63) // 64 * 64
    ws = workspace(lg.device, B * M + B + 2 * B * M * s_pad)
    loss = torch.empty((1,), dtype=torch.float32, device=lg.device)
    grad = torch.empty_like(lg) if want_grad else None
    _launch("ctc_loss_kernels", 0.0, 4.0 * (lg.numel() * (2 + int(want_grad)) + 4 * B * M * s_pad), lib().ispk_attn_ctc_loss_f32,
            lg.data_ptr(), text_len.data_ptr(), mel_len.data_ptr(), blank_logprob, ws.data_ptr(), ws.numel(), loss.data_ptr(),
            _ptr(grad), grad_out, B, M, L, _stream())
    return loss, (grad.view(attn_logits.shape) if grad is not None else None)


def attn_bin_loss(attn_soft: Tensor, attn_hard: Tensor, eps: float = 1e-6, want_grad: bool = False, grad_out: float = 1.0):
    """ispk_attn_bin_loss_f32 -> (loss fp32 [2] = (loss, number of path cells), grad fp32 like attn_soft | None)."""
    _dev(attn_soft, attn_hard)
    assert attn_soft.dtype == torch.float32 and attn_hard.dtype == torch.int16 and attn_soft.shape == attn_hard.shape
    attn_soft, attn_hard = attn_soft.contiguous(), attn_hard.contiguous()
    B, M, L = attn_soft.shape[0], attn_soft.shape[-2], attn_soft.shape[-1]
    loss = torch.empty((2,), dtype=torch.float32, device=attn_soft.device)
    grad = zeros(attn_soft.shape, attn_soft.dtype, attn_soft.device) if want_grad else None
    ws = workspace(attn_soft.device, 2048)
    _launch("bin_loss_kernels", 0.0, 6.0 * attn_soft.numel(), lib().ispk_attn_bin_loss_f32, attn_soft.data_ptr(),
            attn_hard.data_ptr(), eps, ws.data_ptr(), loss.data_ptr(), _ptr(grad), grad_out, B, M, L, _stream())
    return loss, grad


def mel_grad_rows(dmel: Tensor, mask: Optional[Tensor]) -> Tensor:
    """ispk_mel_grad_rows_f32: [B, C, T] gradient of the mel output -> masked rows [B, T, C] for to_mel's backward."""
    _dev(dmel, mask)
    assert dmel.dtype == torch.float32 and dmel.ndim == 3
    dmel = dmel.contiguous()
    B, C, T = dmel.shape
    if mask is not None:
        mask = mask.contiguous()
        assert mask.dtype == torch.bool and mask.shape == (B, T)
    g = torch.empty((B, T, C), dtype=torch.float32, device=dmel.device)
    _launch("mel_grad_rows_kernel", 0.0, 8.0 * dmel.numel(), lib().ispk_mel_grad_rows_f32, dmel.data_ptr(), _ptr(mask),
            g.data_ptr(), B, C, T, _stream())
    return g


def colsum(x: Tensor, row_mask: Optional[Tensor] = None) -> Tensor:
    """ispk_colsum_f32: column sums of a [rows, cols] fp32 matrix (bias gradients) over the rows `row_mask` keeps, fixed order."""
    _dev(x, row_mask)
    x2 = _rows2d(x)
    assert x2.dtype == torch.float32
    rows, cols = x2.shape
    if row_mask is not None:
        row_mask = row_mask.reshape(-1).contiguous()
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    out = torch.empty((cols,), dtype=torch.float32, device=x.device)
    if rows == 0:
        return zero_(out)
    ws = workspace(x.device, 256 * cols)
    _launch("colsum_kernels", 0.0, 4.0 * x2.numel(), lib().ispk_colsum_f32, x2.data_ptr(), x2.stride(0), rows, cols,
            _ptr(row_mask), ws.data_ptr(), ws.numel(), out.data_ptr(), _stream())
    return out


def smallk_wgrad(g: Tensor, x: Tensor) -> Tensor:
    """ispk_smallk_wgrad_f32: out[n, k] = sum_r g[r, n] x[r, k] for a Linear with K <= 8 input features."""
    _dev(g, x)
    g2, x2 = _rows2d(g), _rows2d(x)
    assert g2.dtype == torch.float32 and x2.dtype == torch.float32 and g2.shape[0] == x2.shape[0] and x2.shape[1] <= 8
    rows, N = g2.shape
    K = x2.shape[1]
    out = torch.empty((N, K), dtype=torch.float32, device=g.device)
    if rows == 0:
        return zero_(out)
    ws = workspace(g.device, 256 * N * K)
    _launch("smallk_wgrad_kernels", 2.0 * rows * N * K, 4.0 * (g2.numel() + x2.numel()), lib().ispk_smallk_wgrad_f32, g2.data_ptr(),
            g2.stride(0), x2.data_ptr(), x2.stride(0), rows, N, K, ws.data_ptr(), ws.numel(), out.data_ptr(), _stream())
    return out


def embedding_bwd(ids: Tensor, d_emb: Tensor, vocab: int, padding_idx: int = 0) -> Tensor:
    """ispk_embedding_bwd_f32 -> d_table fp32 [vocab, D]."""
    _dev(ids, d_emb)
    ids = ids.reshape(-1).to(torch.int64).contiguous()
    d2 = _rows2d(d_emb).contiguous()
    assert d2.dtype == torch.float32 and d2.shape[0] == ids.numel()
    out = torch.empty((vocab, d2.shape[1]), dtype=torch.float32, device=d_emb.device)
    _launch("embedding_bwd_kernel", 0.0, 4.0 * d2.numel(), lib().ispk_embedding_bwd_f32, ids.data_ptr(), d2.data_ptr(), ids.numel(),
            d2.shape[1], vocab, padding_idx, out.data_ptr(), out.stride(0), _stream())
    return out


def grad_sqnorm(g: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ispk_grad_sqnorm_f32: sum of squares of a flat fp32 arena -> fp32 [1] (device)."""
    _dev(g, out)
    assert g.dtype == torch.float32 and g.ndim == 1 and g.is_contiguous()
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=g.device)
    part = workspace(g.device, 2048)
    _launch("sqnorm_kernels", 0.0, 4.0 * g.numel(), lib().ispk_grad_sqnorm_f32, g.data_ptr(), g.numel(), part.data_ptr(),
            out.data_ptr(), _stream())
    return out


def set_seed_source(word: Optional[Tensor]) -> None:
    """ispk_set_dropout_seed_source: while set (a one-element int64 DEVICE tensor the caller keeps alive), every dropout kernel
    launched by this process - from the calling thread or from autograd's backward worker - folds that word into its seed
    when it runs: what lets a captured training step draw fresh masks on every replay.  None switches it off."""
    if word is not None:
        _dev(word)
        assert word.dtype == torch.int64 and word.numel() == 1
    _check(lib().ispk_set_dropout_seed_source(None if word is None else word.data_ptr()), "set_dropout_seed_source")


def adam_args(lr: float, betas: tuple, eps: float, weight_decay: float, step: int, max_norm: float = 1.0,
              grad_scale: float = 1.0) -> Tensor:
    """ispk_adam_args_f32 -> the 10 fp32 factors of AdamW step `step` as a pinned host tensor (for a copy to the device
    record that ispk_adamw_f32_dev reads)."""
    buf = (ctypes.c_float * 10)()
    _check(lib().ispk_adam_args_f32(lr, betas[0], betas[1], eps, weight_decay, step, max_norm, grad_scale,
                                    ctypes.cast(buf, ctypes.c_void_p)), "adam_args")
    t = torch.tensor(list(buf), dtype=torch.float32)
    return t.pin_memory() if torch.cuda.is_available() else t


def adamw_dev(p: Tensor, g: Tensor, m: Tensor, v: Tensor, n_decay: int, args_dev: Tensor, grad_sqnorm: Optional[Tensor] = None) -> None:
    """ispk_adamw_f32_dev: `adamw` with the step's factors read from the device record `args_dev` (fp32 [10], adam_args)."""
    _dev(p, g, m, v, args_dev, grad_sqnorm)
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.ndim == 1 and t.is_contiguous() and t.numel() == p.numel()
    assert args_dev.dtype == torch.float32 and args_dev.numel() == 10 and args_dev.is_contiguous()
    _launch("adamw_kernel", 0.0, 28.0 * p.numel(), lib().ispk_adamw_f32_dev, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
            p.numel(), n_decay, args_dev.data_ptr(), _ptr(grad_sqnorm), _stream())


def adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, n_decay: int, lr: float, betas: tuple, eps: float, weight_decay: float,
          step: int, grad_sqnorm: Optional[Tensor] = None, max_norm: float = 1.0, grad_scale: float = 1.0) -> None:
    """ispk_adamw_f32 over flat fp32 arenas (in place)."""
    _dev(p, g, m, v, grad_sqnorm)
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.ndim == 1 and t.is_contiguous() and t.numel() == p.numel()
    _launch("adamw_kernel", 0.0, 28.0 * p.numel(), lib().ispk_adamw_f32, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
            p.numel(), n_decay, lr, betas[0], betas[1], eps, weight_decay, step, _ptr(grad_sqnorm), max_norm, grad_scale,
            _stream())


# ------------------------------------------------------------------------------------------------- Vocos vocoder
VOCODER_HOP = 256             # ispk_istft_head_f32: n_fft 1024, hop 256, padding "same"
VOCODER_TABLE_FLOATS = 2 * 2048 + 1024


def _lengths_ptr(mel_len: Optional[Tensor], B: int) -> Optional[int]:
    if mel_len is None:
        return None
    if mel_len.dtype != torch.int64 or mel_len.shape != (B,) or not mel_len.is_contiguous():
        raise ValueError(f"mel_len: contiguous int64 [{B}], got {mel_len.dtype} {tuple(mel_len.shape)}")
    return mel_len.data_ptr()


def vocoder_unfold(mel: Tensor, mel_len: Optional[Tensor], rows: Tensor, row_mask: Optional[Tensor] = None) -> Tensor:
    """ispk_vocoder_unfold: mel fp32 / fp16 [B, C, T] (any strides) -> the embedding convolution's GEMM rows [B*T, K] (fp32 or
    bf16, K % 8 == 0, K >= 7 C; column j*C + c = tap j of channel c), zero past mel_len; row_mask bool [B*T] (t < mel_len)."""
    _dev(mel, mel_len, rows, row_mask)
    assert mel.ndim == 3 and mel.dtype in (torch.float32, torch.float16)
    B, C, T = mel.shape
    assert rows.ndim == 2 and rows.shape[0] == B * T and rows.stride(1) == 1 and rows.dtype in (torch.float32, torch.bfloat16)
    assert row_mask is None or (row_mask.dtype == torch.bool and row_mask.numel() == B * T and row_mask.is_contiguous())
    K = rows.shape[1]
    ml = _lengths_ptr(mel_len, B)
    if B * T == 0:
        return rows
    _launch(f"vocoder_unfold_kernel<{'f16' if mel.dtype == torch.float16 else 'f32'},"
            f"{'bf16' if rows.dtype == torch.bfloat16 else 'f32'}>", 0.0,
            float(mel.numel() * mel.element_size() + rows.numel() * rows.element_size() + B * T), lib().ispk_vocoder_unfold,
            mel.data_ptr(), int(mel.dtype == torch.float16), mel.stride(0), mel.stride(1), mel.stride(2), ml, rows.data_ptr(),
            int(rows.dtype == torch.bfloat16), rows.stride(0), _ptr(row_mask), B, C, T, K, _stream())
    return rows


def dwconv7_ln(x: Tensor, T: int, weight: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor, mel_len: Optional[Tensor],
               eps: float = 1e-6, out_dtype: torch.dtype = torch.float32, out: Optional[Tensor] = None) -> Tensor:
    """ispk_dwconv7_ln_f32: x fp32 [B*T, D] rows (unit column stride) -> LayerNorm(depthwise conv7(x)) fp32 / bf16 [B*T, D],
    each utterance's frames [0, mel_len) convolved alone, rows past mel_len zero.  weight fp32 [D, 7] contiguous."""
    _dev(x, weight, bias, gamma, beta, mel_len, out)
    assert x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1
    R, D = x.shape
    B = R // T if T > 0 else 0
    assert B * T == R and weight.shape == (D, 7) and weight.is_contiguous()
    if out is None:
        out = torch.empty((R, D), dtype=out_dtype, device=x.device)
    assert out.shape == (R, D) and out.stride(1) == 1 and out.dtype in (torch.float32, torch.bfloat16)
    ml = _lengths_ptr(mel_len, B)
    if R == 0:
        return out
    _launch(f"dwconv7_ln_kernel<{D // 64},{'bf16' if out.dtype == torch.bfloat16 else 'f32'}>", 18.0 * R * D,
            float(R * D * (4 + out.element_size())), lib().ispk_dwconv7_ln_f32, x.data_ptr(), x.stride(0), weight.data_ptr(),
            bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, ml, out.data_ptr(), int(out.dtype == torch.bfloat16),
            out.stride(0), B, T, D, _stream())
    return out


def istft_head(h: Tensor, T: int, mel_len: Optional[Tensor], tables: Tensor, audio: Tensor,
               audio_len: Optional[Tensor] = None) -> Tensor:
    """ispk_istft_head_f32: the head Linear's fp32 rows h [B*T, >= 1026] (log-magnitudes in columns 0-512, phases in 513-1025)
    -> audio fp32 [B, S] (unit stride on S, S >= 256 T; zero from 256 mel_len on) and audio_len int64 [B] = 256 mel_len."""
    _dev(h, mel_len, tables, audio, audio_len)
    assert h.dtype == torch.float32 and h.ndim == 2 and h.stride(1) == 1
    assert audio.dtype == torch.float32 and audio.ndim == 2 and audio.stride(1) == 1
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= VOCODER_TABLE_FLOATS
    B, S = audio.shape
    assert h.shape[0] == B * T
    assert audio_len is None or (audio_len.dtype == torch.int64 and audio_len.shape == (B,) and audio_len.is_contiguous())
    ml = _lengths_ptr(mel_len, B)
    if B == 0:
        return audio
    R = B * T
    _launch("istft_head_kernel", R * 1.25 * (5.0 * 512 * 9 + 20.0 * 513), float(R * 1026 * 4 + B * S * 4),
            lib().ispk_istft_head_f32, h.data_ptr(), h.stride(0), ml, tables.data_ptr(), tables.numel(), audio.data_ptr(),
            audio.stride(0), _ptr(audio_len), B, T, S, _stream())
    return audio


# ------------------------------------------------------------------------------------------------- HiFi-GAN vocoder
HIFIGAN_TILE_ROWS = 128       # ispk_hifigan_tile_rows(): time positions per workgroup of the convolution kernels
HIFIGAN_MAX_CHANNELS = 512    # C_in, C_out: multiples of 32 up to this
HIFIGAN_MAX_KERNEL, HIFIGAN_MAX_DILATION = 11, 12


def _hifigan_rows(x: Tensor, name: str) -> None:
    assert x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1, f"{name}: fp32 rows [R, C] with unit column stride"


def hifigan_conv(x: Tensor, T: int, weight: Tensor, bias: Optional[Tensor], k: int, dilation: int = 1, slope: float = 1.0,
                 resid: Optional[Tensor] = None, out: Optional[Tensor] = None, accumulate: bool = False, scale: float = 1.0,
                 lengths: Optional[Tensor] = None, len_mul: int = 1) -> Tensor:
    """ispk_hifigan_conv_{f32,bf16} by weight.dtype: x fp32 [B*T, C_in] rows -> out fp32 [B*T, C_out] =
    [out +] scale * (bias + Conv1d(k, dilation, "same")(leaky_relu(x, slope)) [+ resid]); weight image [k, C_out, C_in].
    lengths int64 [B]: utterance b has lengths[b] * len_mul valid rows, the rest read and are written as zeros."""
    _dev(x, weight, bias, resid, out, lengths)
    _hifigan_rows(x, "x")
    R, C_in = x.shape
    B = R // T if T > 0 else 0
    assert B * T == R and weight.ndim == 3 and weight.is_contiguous() and weight.shape[0] == k and weight.shape[2] == C_in
    assert weight.dtype in (torch.float32, torch.bfloat16)
    C_out = weight.shape[1]
    assert not accumulate or out is not None, "accumulate needs out="
    if out is None:
        out = torch.empty((R, C_out), dtype=torch.float32, device=x.device)
    _hifigan_rows(out, "out")
    assert out.shape == (R, C_out)
    if resid is not None:
        _hifigan_rows(resid, "resid")
        assert resid.shape == (R, C_out)
    ln = _lengths_ptr(lengths, B)
    if R == 0:
        return out
    bf = weight.dtype == torch.bfloat16
    _launch(f"hifigan_conv_kernel<{'bf16' if bf else 'f32'},{_hifigan_bn(C_out)}>", 2.0 * R * C_out * C_in * k,
            float(R * 4 * (C_in + C_out * (1 + (resid is not None) + bool(accumulate))) + weight.numel() * weight.element_size()),
            lib().ispk_hifigan_conv_bf16 if bf else lib().ispk_hifigan_conv_f32, x.data_ptr(), x.stride(0), weight.data_ptr(),
            _ptr(bias), _ptr(resid), resid.stride(0) if resid is not None else 0, out.data_ptr(), out.stride(0), ln, len_mul, B,
            T, C_in, C_out, k, dilation, slope, scale, int(accumulate), _stream())
    return out


def _hifigan_bn(C_out: int) -> int:
    return 128 if C_out % 128 == 0 else 64 if C_out % 64 == 0 else 32


def hifigan_upsample(x: Tensor, T: int, weight: Tensor, bias: Optional[Tensor], k: int, stride: int, slope: float = 0.1,
                     out: Optional[Tensor] = None, lengths: Optional[Tensor] = None, len_mul: int = 1) -> Tensor:
    """ispk_hifigan_upsample_{f32,bf16} by weight.dtype: x fp32 [B*T, C_in] rows -> out fp32 [B*T*stride, C_out] = bias +
    ConvTranspose1d(k, stride, padding (k - stride) / 2)(leaky_relu(x, slope)); weight image [k, C_out, C_in] (the module's
    [C_in, C_out, k] permuted).  lengths[b] * len_mul valid INPUT rows; output rows past stride times that are zeros."""
    _dev(x, weight, bias, out, lengths)
    _hifigan_rows(x, "x")
    R, C_in = x.shape
    B = R // T if T > 0 else 0
    assert B * T == R and weight.ndim == 3 and weight.is_contiguous() and weight.shape[0] == k and weight.shape[2] == C_in
    assert weight.dtype in (torch.float32, torch.bfloat16)
    C_out = weight.shape[1]
    if out is None:
        out = torch.empty((R * stride, C_out), dtype=torch.float32, device=x.device)
    _hifigan_rows(out, "out")
    assert out.shape == (R * stride, C_out)
    ln = _lengths_ptr(lengths, B)
    if R == 0:
        return out
    bf = weight.dtype == torch.bfloat16
    _launch(f"hifigan_conv_kernel<{'bf16' if bf else 'f32'},{_hifigan_bn(C_out)}>(T)", 2.0 * R * C_out * C_in * k,
            float(R * 4 * (C_in + C_out * stride) + weight.numel() * weight.element_size()),
            lib().ispk_hifigan_upsample_bf16 if bf else lib().ispk_hifigan_upsample_f32, x.data_ptr(), x.stride(0),
            weight.data_ptr(), _ptr(bias), out.data_ptr(), out.stride(0), ln, len_mul, B, T, C_in, C_out, k, stride, slope,
            _stream())
    return out


def hifigan_post(x: Tensor, T: int, weight: Tensor, bias: Tensor, audio: Tensor, audio_len: Optional[Tensor] = None,
                 lengths: Optional[Tensor] = None, len_mul: int = 1, slope: float = 0.01) -> Tensor:
    """ispk_hifigan_post_f32: x fp32 [B*T, C] rows -> audio fp32 [B, S >= T] = tanh(bias + conv7(leaky_relu(x, slope))), zeros
    from lengths[b] * len_mul on; audio_len int64 [B] = lengths[b] * len_mul.  weight fp32 [7, C] contiguous, bias fp32 [1]."""
    _dev(x, weight, bias, audio, audio_len, lengths)
    _hifigan_rows(x, "x")
    assert audio.dtype == torch.float32 and audio.ndim == 2 and (audio.stride(1) == 1 or audio.shape[1] <= 1)
    B, S = audio.shape
    C = x.shape[1]
    assert x.shape[0] == B * T and weight.shape == (7, C) and weight.is_contiguous() and weight.dtype == torch.float32
    assert bias.dtype == torch.float32 and bias.numel() == 1
    assert audio_len is None or (audio_len.dtype == torch.int64 and audio_len.shape == (B,) and audio_len.is_contiguous())
    ln = _lengths_ptr(lengths, B)
    if B == 0:
        return audio
    _launch("hifigan_post_kernel", 14.0 * B * T * C, float(B * T * C * 4 + B * S * 4), lib().ispk_hifigan_post_f32,
            _ptr(x) if x.numel() else None, x.stride(0), weight.data_ptr(), bias.data_ptr(), ln, len_mul, audio.data_ptr(),
            max(audio.stride(0), S), _ptr(audio_len), B, T, S, C, slope, _stream())
    return audio
