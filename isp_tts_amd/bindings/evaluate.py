"""Evaluator kernels (csrc/metrics.hip, csrc/dtw.hip): acoustic metrics, DTW and MCD-DTW."""
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["METRICS_CHUNK", "metrics_workspace_floats", "_mel_strides", "acoustic_metrics", "DTW_MAX_LEN", "DTW_LANES",
           "dtw_workspace_floats", "mcd_dtw_workspace_floats", "dtw", "mcd_dtw"]


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
    _rt._dev(mel_out, mel_target, mel_len, text_len, attn_soft, dct, out)
    if out is None:
        out = torch.empty((3,), dtype=torch.float32, device=mel_len.device)
    assert out.dtype == torch.float32 and out.numel() == 3 and out.is_contiguous()
    B = mel_len.shape[0]
    if B == 0:
        return out.fill_(float("nan"))
    mel_len = _rt._i64(mel_len)
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
        text_len = _rt._i64(text_len)
    ws = torch.empty((_rt.metrics_workspace_floats(B, T),), dtype=torch.float32, device=mel_len.device)
    nbytes = 4.0 * (2 * B * C * T + (attn_soft.numel() if attn_soft is not None else 0))
    _rt._launch("acoustic_metrics_kernels", 2.0 * B * T * C * n_mfcc, nbytes, _rt.lib().ispk_acoustic_metrics_f32,
                _rt._ptr(mel_out), m[2], m[3], m[4], _rt._ptr(mel_target), mt[2], mt[3], mt[4], mel_len.data_ptr(),
                _rt._ptr(text_len) if attn_soft is not None else None, _rt._ptr(attn_soft),
                _rt._ld(attn_soft), attn_soft.stride(1) if attn_soft is not None else 0,
                _rt._ptr(dct), ws.data_ptr(), ws.numel(), out.data_ptr(), B, C, T, L, n_mfcc, _rt._stream())
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
    return _rt.dtw_workspace_floats(B, N, M) + B * (N + M) * kp + 2 * B


def dtw(cost: Tensor, n_len: Tensor, m_len: Tensor, want_path: bool = True):
    """ispk_dtw_f32.  cost fp32 [B, N, M] (unit stride on M), lengths int64 [B] on the device -> (total fp32 [B], steps int32
    [B], path int16 [B, N + M - 1, 2] | None): the cells of the warping path from (0, 0), -1 past `steps`.  No host read."""
    _rt._dev(cost, n_len, m_len)
    assert cost.dtype == torch.float32 and cost.ndim == 3
    if cost.stride(2) != 1:
        cost = cost.contiguous()
    B, N, M = cost.shape
    n_len, m_len = _rt._i64(n_len), _rt._i64(m_len)
    assert n_len.shape == (B,) and m_len.shape == (B,)
    total = torch.empty((B,), dtype=torch.float32, device=cost.device)
    steps = torch.empty((B,), dtype=torch.int32, device=cost.device)
    path = torch.empty((B, N + M - 1, 2), dtype=torch.int16, device=cost.device) if want_path else None
    if B == 0:
        return total, steps, path
    ws = _rt.workspace(cost.device, _rt.dtw_workspace_floats(B, N, M))
    _rt._launch("dtw_kernel", 4.0 * B * N * M, 12.25 * B * N * M, _rt.lib().ispk_dtw_f32, cost.data_ptr(), cost.stride(0), cost.stride(1),
                n_len.data_ptr(), m_len.data_ptr(), total.data_ptr(), steps.data_ptr(), _rt._ptr(path), ws.data_ptr(), ws.numel(), B, N,
                M, _rt._stream())
    return total, steps, path


def mcd_dtw(mel_out: Tensor, mel_out_len: Tensor, mel_target: Tensor, mel_target_len: Tensor, dct: Tensor,
            pitch_out: Optional[Tensor] = None, pitch_target: Optional[Tensor] = None, out: Optional[Tensor] = None,
            cost_out: Optional[Tensor] = None):
    """ispk_mcd_dtw_f32 -> (per_item fp32 [4, B], means fp32 [4]), two views of ONE device buffer of 4 B + 4 floats (`out`,
    when given): rows / elements 0 .. 3 are (mcd_dtw, f0_rmse_cents, vuv_error, length_ratio).  mels fp32 [B, C, T] or
    [B, T, C] under the layout rule of `_mel_strides`, dct fp32 [C, n_mfcc] on the device, lengths int64 [B], pitch fp32
    [B, >= T] in Hz with 0 = unvoiced (both or neither: without them rows 1 and 2 are not written).  `cost_out`: fp32 [B, N, M]
    (contiguous) that receives each item's n_len x m_len costs.  No host read.  B = 0 gives NaN means without a launch."""
    _rt._dev(mel_out, mel_out_len, mel_target, mel_target_len, dct, pitch_out, pitch_target, out, cost_out)
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
    n_len, m_len = _rt._i64(mel_out_len), _rt._i64(mel_target_len)
    if pitch_out is not None:
        assert pitch_out.dtype == torch.float32 and pitch_target.dtype == torch.float32
        assert pitch_out.ndim == 2 and pitch_target.ndim == 2 and pitch_out.shape[0] == B and pitch_target.shape[0] == B
        if pitch_out.shape[1] < N or pitch_target.shape[1] < M:
            raise ValueError(f"pitch tracks {tuple(pitch_out.shape)} / {tuple(pitch_target.shape)} are shorter than the mels")
        if pitch_out.stride(1) != 1:
            pitch_out = pitch_out.contiguous()
        if pitch_target.stride(1) != 1:
            pitch_target = pitch_target.contiguous()
    ws = _rt.workspace(mel_out.device, _rt.mcd_dtw_workspace_floats(B, N, M, n_mfcc))
    if cost_out is not None:
        assert cost_out.dtype == torch.float32 and cost_out.shape == (B, N, M) and cost_out.is_contiguous()
    _rt._launch("mcd_dtw_kernels", 2.0 * B * (N + M) * C * n_mfcc + 3.0 * B * N * M * n_mfcc, 8.25 * B * N * M,
                _rt.lib().ispk_mcd_dtw_f32, mel_out.data_ptr(), m[2], m[3], m[4], mel_target.data_ptr(), mt[2], mt[3], mt[4],
                dct.data_ptr(), n_len.data_ptr(), m_len.data_ptr(), _rt._ptr(pitch_out), _rt._ld(pitch_out), _rt._ptr(pitch_target),
                _rt._ld(pitch_target), ws.data_ptr(), ws.numel(), per_item.data_ptr(), means.data_ptr(), _rt._ptr(cost_out), B, C, N, M,
                n_mfcc, _rt._stream())
    return per_item, means
