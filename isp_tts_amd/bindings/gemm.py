"""GEMM wrappers (csrc/gemm.hip): Linear layers with their epilogues, to_mel, the small-shape and batched forms."""
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["_splitk_layout_ok", "gemm", "gemm_lnin", "_gemm_label", "_gemm_bytes", "to_mel", "linear_small", "linear",
           "gemm_batched"]


def _splitk_layout_ok(c2: Tensor, bias: Optional[Tensor], r2: Optional[Tensor], flags: int) -> bool:
    """The pointer / leading-dimension half of vec_epilogue_ok (csrc/gemm.hip), which ispk_gemm_bf16_splitk requires on
    top of its plan (the plan sees only M, N, K and flags).  Views that fail it (an offset `out=`, a bias slice off 16 bytes,
    an odd row stride) go to ispk_gemm_bf16, whose other kernels take any layout."""
    c_align = 8 if flags & _rt.EP_OUT_BF16 else 16
    r_align = 8 if flags & _rt.EP_RESID_BF16 else 16
    return (c2.stride(0) % 4 == 0 and c2.data_ptr() % c_align == 0 and
            (r2 is None or (r2.stride(0) % 4 == 0 and r2.data_ptr() % r_align == 0)) and
            (bias is None or bias.data_ptr() % 16 == 0))


def gemm(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
         mask: Optional[Tensor] = None, flags: int = 0, out: Optional[Tensor] = None,
         out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """C[..., N] = epilogue(a[..., K] @ w[N, K]^T)  (ispk_gemm_f32 / ispk_gemm_bf16 by a.dtype)."""
    _rt._dev(a, w, bias, resid, mask, out)
    a2 = _rt._rows2d(a)
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
        r2 = _rt._rows2d(resid)
        assert r2.shape == (M, N)
    if mask is not None:
        mask = _rt._mask1d(mask)
        assert mask.dtype == torch.bool
    if M == 0:      # nothing to compute; the C entries would refuse the NULL data_ptr() torch gives an empty tensor
        return out
    if bf16:
        if out.dtype == torch.bfloat16:
            flags |= _rt.EP_OUT_BF16
        if r2 is not None and r2.dtype == torch.bfloat16:
            flags |= _rt.EP_RESID_BF16
        fn = _rt.lib().ispk_gemm_bf16
        ks = _rt.lib().ispk_gemm_bf16_splitk_plan(M, N, K, flags) if M < 2048 and K >= 512 else 1
        if ks > 1 and _splitk_layout_ok(c2, bias, r2, flags):
            # few rows, long K: K slices on separate workgroups + one combine pass (ispk_gemm_bf16_splitk)
            ws = torch.empty((ks * M * N,), dtype=torch.float32, device=a.device)
            _rt._launch(f"gemm_bf16_splitk<{ks}>", 2.0 * M * N * K, _gemm_bytes(a2, w, out, r2) + 8.0 * ks * M * N, _rt.lib().ispk_gemm_bf16_splitk,
                        a2.data_ptr(), a2.stride(0), w.data_ptr(), w.stride(0), c2.data_ptr(), c2.stride(0), _rt._ptr(bias), _rt._ptr(r2),
                        _rt._ld(r2), _rt._ptr(mask), M, N, K, flags, ws.data_ptr(), ks, _rt._stream())
            return out
    else:
        assert out.dtype == torch.float32 and (r2 is None or r2.dtype == torch.float32)
        fn = _rt.lib().ispk_gemm_f32
    _rt._launch(_gemm_label(bf16, M, N, K), 2.0 * M * N * K, _gemm_bytes(a2, w, out, r2), fn, a2.data_ptr(), a2.stride(0),
                w.data_ptr(), w.stride(0), c2.data_ptr(), c2.stride(0), _rt._ptr(bias), _rt._ptr(r2),
                _rt._ld(r2), _rt._ptr(mask), M, N, K, flags, 0, 0, _rt._stream())
    return out


def gemm_lnin(x: Tensor, stats: Optional[Tensor], ln_weight: Tensor, ln_bias: Tensor, w: Tensor,
              bias: Optional[Tensor] = None, mask: Optional[Tensor] = None, flags: int = 0,
              out_dtype: torch.dtype = torch.bfloat16, ln_eps: float = 1e-5) -> Tensor:
    """ispk_gemm_bf16_lnin: C[..., N] = epilogue(bf16(LayerNorm(x)) @ w[N, K]^T) with x fp32 [..., K]; the rows'
    (mean, rstd) come from `stats` (written by `ffn_prenorm` / `ffn_prenorm2`) or, with stats None, are computed by
    the kernel itself."""
    _rt._dev(x, stats, ln_weight, ln_bias, w, bias, mask)
    assert x.dtype == torch.float32 and w.dtype == torch.bfloat16
    x2 = _rt._rows2d(x)
    M, K = x2.shape
    N = w.shape[0]
    assert w.shape == (N, K) and w.stride(1) == 1
    assert stats is None or (stats.dtype == torch.float32 and stats.shape == (M, 2) and stats.is_contiguous())
    if out_dtype == torch.bfloat16:
        flags |= _rt.EP_OUT_BF16
    out = torch.empty((*x.shape[:-1], N), dtype=out_dtype, device=x.device)
    mask = _rt._mask1d(mask)
    nb = x2.numel() * 4 + (stats.numel() * 4 if stats is not None else 0) + w.numel() * 2 + out.numel() * out.element_size()
    _rt._launch(f"gemm_bf16_panel_kernel<{K // 64},lnin>", 2.0 * M * N * K, float(nb), _rt.lib().ispk_gemm_bf16_lnin, x2.data_ptr(),
                x2.stride(0), _rt._ptr(stats), ln_weight.data_ptr(), ln_bias.data_ptr(), ln_eps, w.data_ptr(), w.stride(0),
                out.data_ptr(), N, _rt._ptr(bias), 0, 0, _rt._ptr(mask), M, N, K, flags, _rt._stream())
    return out


def _gemm_label(bf16: bool, M: int, N: int, K: int) -> str:
    if bf16:
        return "gemm_bf16_kernel"
    t = _rt.lib().ispk_gemm_f32_tile(M, N, K)
    return f"gemm_f32_kernel<{t // 10},{t % 10}>"


def _gemm_bytes(a2: Tensor, w: Tensor, out: Tensor, r2: Optional[Tensor]) -> float:
    n = a2.numel() * a2.element_size() + w.numel() * w.element_size() + out.numel() * out.element_size()
    return float(n + (r2.numel() * r2.element_size() if r2 is not None else 0))


def to_mel(dec: Tensor, weight: Tensor, bias: Tensor, mask: Optional[Tensor]) -> Tensor:
    """mel[B, C, T] = mask[b,t] * (dec[B,T,D] @ weight[C,D]^T + bias[C])  — Linear + transpose + mask of
    model.py:167-168 as ONE GEMM with swapped operands: lanes run along the mel-frame axis T, so the transposed
    output is written with coalesced 128-B segments."""
    _rt._dev(dec, weight, bias, mask)
    B, T, D = dec.shape
    C = weight.shape[0]
    x2 = _rt._rows2d(dec)
    out = torch.empty((B, C, T), dtype=torch.float32, device=dec.device)
    if dec.dtype == torch.bfloat16 and D in (256, 384) and C % 4 == 0 and bias is not None:
        # bf16, K = 256 / 384: the panel GEMM with frames as rows and the transposed per-batch store (ISPK_EP_ROWS_T)
        flags = _rt.EP_ROWS_T
        if mask is not None:
            mask = _rt._mask1d(mask)
            flags |= _rt.EP_MASK_OUT
        _rt._launch("gemm_bf16_kernel", 2.0 * C * B * T * D, _gemm_bytes(x2, weight, out, None), _rt.lib().ispk_gemm_bf16,
                    x2.data_ptr(), x2.stride(0), weight.data_ptr(), weight.stride(0), out.data_ptr(), T, _rt._ptr(bias), None, 0,
                    _rt._ptr(mask), B * T, C, D, flags, T, C * T, _rt._stream())
        return out
    flags = _rt.EP_BIAS_ROW | _rt.EP_MASK_COL
    if mask is not None:
        mask = _rt._mask1d(mask)
        flags |= _rt.EP_MASK_OUT
    fn = _rt.lib().ispk_gemm_bf16 if dec.dtype == torch.bfloat16 else _rt.lib().ispk_gemm_f32
    _rt._launch(_gemm_label(dec.dtype == torch.bfloat16, C, B * T, D), 2.0 * C * B * T * D, _gemm_bytes(x2, weight, out, None),
                fn, weight.data_ptr(), weight.stride(0), x2.data_ptr(), x2.stride(0), out.data_ptr(), T, _rt._ptr(bias), None, 0,
                _rt._ptr(mask), C, B * T, D, flags, T, C * T, _rt._stream())
    return out


def linear_small(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
                 act: int = 0) -> Tensor:
    """ispk_linear_small_f32: any K / N, fp32.  `w` may be a column slice of a wider weight (stride kept)."""
    _rt._dev(a, w, bias, resid)
    assert a.dtype == torch.float32 and w.dtype == torch.float32 and w.stride(1) == 1
    a2 = _rt._rows2d(a)
    M, K = a2.shape
    N = w.shape[0]
    assert w.shape[1] == K
    out = torch.empty((*a.shape[:-1], N), dtype=torch.float32, device=a.device)
    r2 = _rt._rows2d(resid) if resid is not None else None
    _rt._launch("linear_small_kernel", 2.0 * M * N * K, 4.0 * (M * K + N * K + M * N), _rt.lib().ispk_linear_small_f32,
                a2.data_ptr(), a2.stride(0), w.data_ptr(), w.stride(0), _rt._ptr(bias), _rt._ptr(r2),
                _rt._ld(r2), out.data_ptr(), N, M, N, K, act, _rt._stream())
    return out


def linear(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, act: int = 0) -> Tensor:
    """nn.Linear on the device: MFMA GEMM when the shape allows (K % 8 == 0, enough rows), else the small kernel."""
    K = w.shape[1]
    rows = a.numel() // K
    if a.dtype == torch.float32 and (K % 8 != 0 or rows * w.shape[0] < 64 * 64 or w.stride(0) % 4 != 0
                                     or w.data_ptr() % 16 != 0):
        return _rt.linear_small(a, w, bias, None, act)
    return _rt.gemm(a, w, bias=bias, flags=act)


def gemm_batched(a: Tensor, w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ispk_gemm_f32_batched: C[i] = a[i] @ w[i]^T for a [batch, M, K], w [batch, N, K] (fp32, unit column strides)
    -> [batch, M, N] (`out`: a view with unit column stride)."""
    _rt._dev(a, w, out)
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
    _rt._launch("gemm_f32_kernel<batched>", 2.0 * batch * M * N * K, 4.0 * (a.numel() + w.numel() + out.numel()),
                _rt.lib().ispk_gemm_f32_batched, a.data_ptr(), a.stride(1), a.stride(0), w.data_ptr(), w.stride(1), w.stride(0),
                out.data_ptr(), out.stride(1), out.stride(0), batch, M, N, K, _rt._stream())
    return out
