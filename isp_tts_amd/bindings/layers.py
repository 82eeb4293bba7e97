"""The transformer layer's kernels: LayerNorm, ALiBi multi-query attention, the feed-forward block and the bf16 cast, and the
split-fp16 forms of the layer (csrc/norm.hip, attention.hip, ffn.hip, ffn2.hip, split.hip)."""
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["layernorm", "ffn_pack_w2", "ffn_fused", "ffn_prenorm", "ffn_chunk_w2", "ffn_prenorm2", "chunk_k16", "attn_out_ffn",
           "ffn_prenorm2_split", "alibi_mqa_attention_raw", "alibi_mqa_attention", "attn_block_short", "split_f16", "layernorm_split", "_split_label",
           "gemm_split", "to_mel_split", "conv5_padded_split", "alibi_mqa_attention_split", "cast_bf16"]


def layernorm(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], ada_scale: Optional[Tensor] = None,
              ada_shift: Optional[Tensor] = None, rows_per_batch: int = 1, row_mask: Optional[Tensor] = None,
              eps: float = 1e-5, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_layernorm_f32[_bf16].  x fp32 [..., D]; ada_* [Bc, D] with Bc == batch or 1 (broadcast)."""
    _rt._dev(x, gamma, beta, ada_scale, ada_shift, row_mask)
    assert x.dtype == torch.float32
    x2 = _rt._rows2d(x)
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
        row_mask = _rt._mask1d(row_mask)
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    fn = _rt.lib().ispk_layernorm_f32 if out_dtype == torch.float32 else _rt.lib().ispk_layernorm_f32_bf16
    label = f"layernorm_vec_kernel<{D // 128}>" if D % 128 == 0 and D <= 512 else f"layernorm_kernel<{D // 64}>"
    _rt._launch(label, 0.0, float(rows) * D * (4 + y.element_size()), fn, x2.data_ptr(),
                x2.stride(0), _rt._ptr(gamma), _rt._ptr(beta), _rt._ptr(ada_scale), _rt._ptr(ada_shift), ada_stride, rows_per_batch,
                _rt._ptr(row_mask), y.data_ptr(), D, rows, D, eps, _rt._stream())
    return y


def cast_bf16(x: Tensor) -> Tensor:
    _rt._dev(x)
    x2 = _rt._rows2d(x)
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _rt._launch("cast_bf16_kernel", 0.0, 6.0 * x2.numel(), _rt.lib().ispk_cast_f32_bf16, x2.data_ptr(), x2.stride(0),
                y.data_ptr(), x2.shape[1], x2.shape[0], x2.shape[1], _rt._stream())
    return y


# ------------------------------------------------------------------------------------------------- feed-forward block
def ffn_pack_w2(w2: Tensor) -> Tensor:
    """ispk_ffn_pack_w2_bf16: W2 bf16 [D, inner] -> packed [inner/32, D, 32] (one-time weight staging for ffn_fused)."""
    _rt._dev(w2)
    assert w2.dtype == torch.bfloat16 and w2.dim() == 2 and w2.stride(1) == 1
    D, Fi = w2.shape
    out = torch.empty((Fi // 32, D, 32), dtype=torch.bfloat16, device=w2.device)
    _rt._launch("ffn_pack_w2_kernel", 0.0, 4.0 * D * Fi, _rt.lib().ispk_ffn_pack_w2_bf16, w2.data_ptr(), w2.stride(0), D, Fi,
                out.data_ptr(), _rt._stream())
    return out


def ffn_fused(x: Tensor, w1: Tensor, w2: Tensor, resid: Optional[Tensor] = None, mask: Optional[Tensor] = None,
              bias1: Optional[Tensor] = None, bias2: Optional[Tensor] = None, flags: int = 0) -> Tensor:
    """ispk_ffn_bf16: out fp32 [..., D] = [mask] * (resid + gelu(x @ w1^T + bias1) @ w2^T + bias2), x / w1 / w2 bf16.
    w2 is either [D, inner] (nn.Linear layout) or the 3-D packed image from `ffn_pack_w2` (faster)."""
    _rt._dev(x, w1, w2, resid, mask, bias1, bias2)
    assert x.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16
    x2 = _rt._rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert w1.shape == (Fi, D) and w1.stride(1) == 1
    packed = w2.dim() == 3
    if packed:
        assert w2.shape == (Fi // 32, D, 32) and w2.is_contiguous()
    else:
        assert w2.shape == (D, Fi) and w2.stride(1) == 1
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    r2 = _rt._rows2d(resid) if resid is not None else None
    mask = _rt._mask1d(mask)
    nb = x2.numel() * 2 + (w1.numel() + w2.numel()) * 2 + out.numel() * 4 + (r2.numel() * 4 if r2 is not None else 0)
    _rt._launch(f"ffn_bf16_kernel<{D // 64}>", 4.0 * R * D * Fi, float(nb), _rt.lib().ispk_ffn_bf16, x2.data_ptr(), x2.stride(0),
                w1.data_ptr(), w1.stride(0), _rt._ptr(bias1), w2.data_ptr(), 0 if packed else w2.stride(0), _rt._ptr(bias2), _rt._ptr(r2),
                _rt._ld(r2), _rt._ptr(mask), out.data_ptr(), D, R, D, Fi, flags, _rt._stream())
    return out


def ffn_prenorm(x: Tensor, norm_weight: Tensor, norm_bias: Tensor, w1: Tensor, w2p: Tensor, mask: Optional[Tensor] = None,
                bias2: Optional[Tensor] = None, flags: int = 0, norm_eps: float = 1e-5, want_stats: bool = False,
                stats_eps: float = 1e-5):
    """ispk_ffn_bf16_prenorm: out fp32 [..., D] = [mask] * (x + gelu(LN(x) @ w1^T) @ w2^T + bias2) from the fp32 rows x
    (LayerNorm input AND residual); with `want_stats` also the (mean, rstd) of the output rows, fp32 [rows, 2]."""
    _rt._dev(x, norm_weight, norm_bias, w1, w2p, mask, bias2)
    assert x.dtype == torch.float32 and w1.dtype == torch.bfloat16 and w2p.dtype == torch.bfloat16
    x2 = _rt._rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert w1.shape == (Fi, D) and w1.stride(1) == 1 and w2p.shape == (Fi // 32, D, 32) and w2p.is_contiguous()
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    stats = torch.empty((R, 2), dtype=torch.float32, device=x.device) if want_stats else None
    mask = _rt._mask1d(mask)
    nb = x2.numel() * 8 + (w1.numel() + w2p.numel()) * 2 + out.numel() * 4 + (R * 8 if want_stats else 0)
    _rt._launch(f"ffn_bf16_kernel<{D // 64}>", 4.0 * R * D * Fi, float(nb), _rt.lib().ispk_ffn_bf16_prenorm, x2.data_ptr(),
                x2.stride(0), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w1.stride(0),
                w2p.data_ptr(), _rt._ptr(bias2), _rt._ptr(mask), out.data_ptr(), D, R, D, Fi, flags, _rt._ptr(stats), stats_eps, _rt._stream())
    return (out, stats) if want_stats else out


def ffn_chunk_w2(w2: Tensor) -> Tensor:
    """ispk_ffn_chunk_w2_bf16: W2 bf16 [D, inner] -> chunk-contiguous [inner/32, D, 32] (weight staging for ffn_prenorm2)."""
    _rt._dev(w2)
    assert w2.dtype == torch.bfloat16 and w2.dim() == 2 and w2.stride(1) == 1
    D, Fi = w2.shape
    out = torch.empty((Fi // 32, D, 32), dtype=torch.bfloat16, device=w2.device)
    _rt._launch("ffn_chunk_w2_kernel", 0.0, 4.0 * D * Fi, _rt.lib().ispk_ffn_chunk_w2_bf16, w2.data_ptr(), w2.stride(0), D, Fi,
                out.data_ptr(), _rt._stream())
    return out


def ffn_prenorm2(x: Tensor, norm_weight: Tensor, norm_bias: Tensor, w1: Tensor, w2c: Tensor, mask: Optional[Tensor] = None,
                 flags: int = 0, norm_eps: float = 1e-5, want_stats: bool = False, stats_eps: float = 1e-5):
    """ispk_ffn_bf16_prenorm2 (dim 384, eight-wave kernel): out fp32 [..., D] = [mask] * (x + gelu(LN(x) @ w1^T) @ w2^T) from the
    fp32 rows x; with `want_stats` also the (mean, rstd) of the output rows, fp32 [rows, 2].  w2c = `ffn_chunk_w2(w2)`."""
    _rt._dev(x, norm_weight, norm_bias, w1, w2c, mask)
    assert x.dtype == torch.float32 and w1.dtype == torch.bfloat16 and w2c.dtype == torch.bfloat16
    x2 = _rt._rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert w1.shape == (Fi, D) and w1.is_contiguous() and w2c.shape == (Fi // 32, D, 32) and w2c.is_contiguous()
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    stats = torch.empty((R, 2), dtype=torch.float32, device=x.device) if want_stats else None
    mask = _rt._mask1d(mask)
    nb = x2.numel() * 8 + (w1.numel() + w2c.numel()) * 2 + out.numel() * 4 + (R * 8 if want_stats else 0)
    _rt._launch("ffn2_bf16_kernel<0>", 4.0 * R * D * Fi, float(nb), _rt.lib().ispk_ffn_bf16_prenorm2, x2.data_ptr(),
                x2.stride(0), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(), _rt._ptr(mask),
                out.data_ptr(), D, R, D, Fi, flags, _rt._ptr(stats), stats_eps, _rt._stream())
    return (out, stats) if want_stats else out


def chunk_k16(w: Tensor) -> Tensor:
    """ispk_chunk_k16_bf16: W bf16 [N, K] -> k-step chunks [K/16, N, 16] (weight staging for attn_out_ffn's q/kv epilogue)."""
    _rt._dev(w)
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    out = torch.empty((K // 16, N, 16), dtype=torch.bfloat16, device=w.device)
    _rt._launch("chunk_k16_kernel", 0.0, 4.0 * N * K, _rt.lib().ispk_chunk_k16_bf16, w.data_ptr(), w.stride(0), N, K, out.data_ptr(),
                _rt._stream())
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
    _rt._dev(x, attn_out, woc, norm_weight, norm_bias, w1, w2c, mask)
    assert x.dtype == torch.float32 and attn_out.dtype == torch.bfloat16 and w1.dtype == torch.bfloat16
    assert woc.dtype == torch.bfloat16 and w2c.dtype == torch.bfloat16
    x2, o2 = _rt._rows2d(x), _rt._rows2d(attn_out)
    R, D = x2.shape
    Fi = w1.shape[0]
    assert o2.shape == (R, D) and woc.shape == (D // 32, D, 32) and woc.is_contiguous()
    assert w1.shape == (Fi, D) and w1.is_contiguous() and w2c.shape == (Fi // 32, D, 32) and w2c.is_contiguous()
    out = torch.empty((*x.shape[:-1], D), dtype=torch.float32, device=x.device)
    stats = torch.empty((R, 2), dtype=torch.float32, device=x.device) if want_stats else None
    flags = 0
    if mask is not None:
        mask = _rt._mask1d(mask)
        flags = _rt.EP_MASK_ACC | _rt.EP_MASK_OUT
    nb = x2.numel() * 4 + o2.numel() * 2 + (woc.numel() + w1.numel() + w2c.numel()) * 2 + out.numel() * 4 + (R * 8 if want_stats else 0)
    if final_norm is not None:
        assert not want_stats and next_qkv is None
        fw, fb, feps, fmask, fdtype = final_norm
        _rt._dev(fw, fb)
        assert fdtype in (torch.float32, torch.bfloat16)
        ln = torch.empty(x.shape, dtype=fdtype, device=x.device)
        outp = out if want_out else None
        _rt._launch("ffn2_bf16_kernel<50>", 4.0 * R * D * Fi + 2.0 * R * D * D,
                    float(nb - (0 if want_out else out.numel() * 4) + ln.numel() * ln.element_size()), _rt.lib().ispk_attn_out_ffn_norm_bf16,
                    x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(), norm_weight.data_ptr(), norm_bias.data_ptr(),
                    norm_eps, w1.data_ptr(), w2c.data_ptr(), _rt._ptr(mask), _rt._ptr(outp), D, R, D, Fi, flags, fw.data_ptr(), fb.data_ptr(), feps,
                    int(bool(fmask) and mask is not None), ln.data_ptr(), D, int(fdtype == torch.bfloat16), _rt._stream())
        return outp, ln
    if next_qkv is not None:
        assert not want_stats
        ng, nbeta, neps, wqc = next_qkv
        _rt._dev(ng, nbeta, wqc)
        assert wqc.dtype == torch.bfloat16 and wqc.shape == (D // 16, 512, 16) and wqc.is_contiguous()
        qkv = torch.empty((*x.shape[:-1], 512), dtype=torch.bfloat16, device=x.device)
        _rt._launch("ffn2_bf16_kernel<51>", 4.0 * R * D * Fi + 2.0 * R * D * D + 2.0 * R * D * 512, float(nb + wqc.numel() * 2 + R * 1024),
                    _rt.lib().ispk_attn_out_ffn_qkv_bf16, x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(),
                    norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(), _rt._ptr(mask), out.data_ptr(), D,
                    R, D, Fi, flags, ng.data_ptr(), nbeta.data_ptr(), neps, wqc.data_ptr(), qkv.data_ptr(), 512, _rt._stream())
        return out, qkv
    _rt._launch("ffn2_bf16_kernel<50>", 4.0 * R * D * Fi + 2.0 * R * D * D, float(nb), _rt.lib().ispk_attn_out_ffn_bf16, x2.data_ptr(),
                x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps,
                w1.data_ptr(), w2c.data_ptr(), _rt._ptr(mask), out.data_ptr(), D, R, D, Fi, flags, _rt._ptr(stats), stats_eps, _rt._stream())
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
    _rt._dev(x, norm_weight, norm_bias, w1, w2c, mask)
    assert x.dtype == torch.float32 and w1.dtype == torch.bfloat16 and w2c.dtype == torch.bfloat16
    x2 = _rt._rows2d(x)
    R, D = x2.shape
    Fi = w1.shape[0]
    parts = torch.empty((splits, R, D), dtype=torch.float32, device=x.device)   # per call: graph instances may run side by side
    if attn_proj is not None:
        o, woc = attn_proj
        _rt._dev(o, woc)
        o2 = _rt._rows2d(o)
        assert o.dtype == torch.bfloat16 and o2.shape == (R, D) and woc.dtype == torch.bfloat16 and woc.shape == (D // 32, D, 32)
        mflat = _rt._mask1d(mask)
        _rt._launch("ffn2_bf16_kernel<21>", (4.0 * R * D * Fi) + 2.0 * R * D * D * splits,
                    float((x2.numel() * 4 + o2.numel() * 2 + woc.numel() * 2) * splits + (w1.numel() + w2c.numel()) * 2 + splits * R * D * 4),
                    _rt.lib().ispk_attn_out_ffn_split_bf16, x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), woc.data_ptr(),
                    norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(), _rt._ptr(mflat),
                    _rt.EP_MASK_ACC if mflat is not None else 0, parts.data_ptr(), R * D, splits, R, D, Fi, _rt._stream())
    else:
        nbytes = x2.numel() * 4 * splits + (w1.numel() + w2c.numel()) * 2 + splits * R * D * 4
        _rt._launch("ffn2_bf16_kernel<20>", 4.0 * R * D * Fi, float(nbytes), _rt.lib().ispk_ffn_bf16_prenorm2_split, x2.data_ptr(),
                    x2.stride(0), norm_weight.data_ptr(), norm_bias.data_ptr(), norm_eps, w1.data_ptr(), w2c.data_ptr(),
                    parts.data_ptr(), R * D, splits, R, D, Fi, _rt._stream())
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    mask = _rt._mask1d(mask)
    ln = None
    nw = nb = None
    neps, nmask, nbf16 = 1e-5, 0, 0
    if next_norm is not None:
        nw, nb, neps, apply_mask, ndtype = next_norm
        ln = torch.empty(x.shape, dtype=ndtype, device=x.device)
        nmask, nbf16 = int(bool(apply_mask) and mask is not None), int(ndtype == torch.bfloat16)
    _rt._launch("ffn_combine_ln_kernel", 0.0, float(R * D * 4 * (2 + splits) + (R * D * ln.element_size() if ln is not None else 0)),
                _rt.lib().ispk_ffn_combine_ln_f32, None if attn_proj is not None else x2.data_ptr(), x2.stride(0), parts.data_ptr(), R * D,
                splits, _rt._ptr(mask), y.data_ptr(),
                D, _rt._ptr(nw), _rt._ptr(nb), neps, nmask, _rt._ptr(ln), D, nbf16, R, D, _rt._stream())
    return y, ln


# ------------------------------------------------------------------------------------------------- attention
def alibi_mqa_attention_raw(q: Tensor, ldq: int, k: Tensor, v: Tensor, ldkv: int, slopes: Tensor,
                            key_len: Optional[Tensor], B: int, N: int, heads: int, q_tiles: int = 0) -> Tensor:
    """ispk_alibi_mqa_attn_*: q is any tensor whose storage holds [B][N][H*64] rows at leading stride ldq starting at
    q.data_ptr(); k / v likewise [B][N][64] at stride ldkv.  Returns the merged heads [B, N, H*64]."""
    _rt._dev(q, k, v, slopes, key_len)
    out = torch.empty((B, N, heads * 64), dtype=q.dtype, device=q.device)
    if B == 0:      # nothing to compute; the C entries would refuse the NULL data_ptr() torch gives an empty tensor
        return out
    key_len = _rt._i64(key_len)
    slopes = slopes.to(torch.float32).contiguous()
    es = q.element_size()
    if es == 4:
        label = "attn_f32_kernel" + ("<384,16>" if heads <= 3 else "<768>" if heads <= 6 else "<1024>")
    else:
        label = "attn_bf16_kernel" + ("<768>" if heads <= 6 else "<1024>")
    flops, nbytes = 256.0 * B * N * N * heads, float(B) * N * (2 * heads * 64 + 128) * es
    if q_tiles:   # explicit query tiles per workgroup (bf16 kernel only; 0 = the launcher's own choice)
        assert es == 2
        _rt._launch(label, flops, nbytes, _rt.lib().ispk_alibi_mqa_attn_bf16_tiles, q.data_ptr(), ldq, k.data_ptr(), v.data_ptr(),
                    ldkv, slopes.data_ptr(), _rt._ptr(key_len), out.data_ptr(), heads * 64, B, N, heads, q_tiles, _rt._stream())
        return out
    fn = _rt.lib().ispk_alibi_mqa_attn_f32 if es == 4 else _rt.lib().ispk_alibi_mqa_attn_bf16
    _rt._launch(label, flops, nbytes, fn, q.data_ptr(), ldq, k.data_ptr(), v.data_ptr(), ldkv,
                slopes.data_ptr(), _rt._ptr(key_len), out.data_ptr(), heads * 64, B, N, heads, _rt._stream())
    return out


def alibi_mqa_attention(qkv: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor], q_tiles: int = 0) -> Tensor:
    """qkv [B, N, H*64 + 128] = [Q | K | V] (the fused to_q / to_kv projection) -> merged heads [B, N, H*64]."""
    B, N, W = qkv.shape
    assert W == heads * 64 + 128 and qkv.is_contiguous()
    return _rt.alibi_mqa_attention_raw(qkv, W, qkv[..., heads * 64:], qkv[..., heads * 64 + 64:], W, slopes, key_len, B, N,
                                       heads, q_tiles)


def attn_block_short(x: Optional[Tensor], wqkv_c: Optional[Tensor], qkv: Optional[Tensor], heads: int, slopes: Tensor,
                     key_len: Optional[Tensor], wo_c: Tensor, resid: Tensor, mask: Optional[Tensor]):
    """ispk_attn_block_short_bf16: one attention block at N <= 128 positions in one launch -> (out fp32 [B, N, D], qkv bf16
    [B, N, D + 128]), D = heads * 64 in {256, 384}.  Either `x` (bf16 [B, N, D], the normalised rows) with wqkv_c =
    `chunk_k16([Wq; Wkv])` - the q/kv rows are computed and returned - or `qkv` (finished rows; x and wqkv_c None).
    wo_c = `chunk_k16(Wo)`; out = resid + mask * (attention @ Wo^T), bit for bit what gemm -> alibi_mqa_attention -> gemm give."""
    _rt._dev(x, wqkv_c, qkv, slopes, key_len, wo_c, resid, mask)
    D = heads * 64
    src = x if x is not None else qkv
    B, N = src.shape[:2]
    assert (x is None) != (qkv is None) and src.dim() == 3 and src.dtype == torch.bfloat16 and src.is_contiguous()
    assert resid.dtype == torch.float32 and resid.shape == (B, N, D) and resid.is_contiguous()
    assert wo_c.dtype == torch.bfloat16 and wo_c.shape == (D // 16, D, 16) and wo_c.is_contiguous()
    if x is not None:
        assert x.shape == (B, N, D) and wqkv_c.dtype == torch.bfloat16 and wqkv_c.shape == (D // 16, D + 128, 16) and wqkv_c.is_contiguous()
        qkv = torch.empty((B, N, D + 128), dtype=torch.bfloat16, device=x.device)
    else:
        assert qkv.shape == (B, N, D + 128)
    out = torch.empty((B, N, D), dtype=torch.float32, device=src.device)
    if B == 0:
        return out, qkv
    mask = _rt._mask1d(mask)
    assert mask is None or (mask.numel() == B * N and mask.element_size() == 1)
    key_len = _rt._i64(key_len)
    slopes = slopes.to(torch.float32).contiguous()
    R = B * N
    flops = 256.0 * B * N * N * heads + 2.0 * R * D * D + (2.0 * R * D * (D + 128) if x is not None else 0.0)
    nbytes = float(R) * (2 * (D + 128) + 8 * D + (2 * D if x is not None else 0)) + 2.0 * D * D + (2.0 * D * (D + 128) if x is not None else 0.0)
    _rt._launch(f"attn_block_short_kernel<{heads}>", flops, nbytes, _rt.lib().ispk_attn_block_short_bf16, _rt._ptr(x), D,
                _rt._ptr(wqkv_c), qkv.data_ptr(), D + 128, slopes.data_ptr(), _rt._ptr(key_len), wo_c.data_ptr(), resid.data_ptr(),
                D, _rt._ptr(mask), out.data_ptr(), D, B, N, heads, _rt._stream())
    return out, qkv


# ------------------------------------------------------------------------------------------------- split-fp16 (parity-grade fast path)
# A "split" tensor is a torch.float16 tensor [2, *shape]: plane 0 = hi = fp16(v), plane 1 = lo = fp16(v - hi).
def split_f16(x: Tensor) -> Tensor:
    """ispk_split_f16: fp32 [..., C] (unit inner stride) -> split planes fp16 [2, ..., C]."""
    _rt._dev(x)
    assert x.dtype == torch.float32
    x2 = _rt._rows2d(x)
    rows, cols = x2.shape
    out = torch.empty((2, *x.shape), dtype=torch.float16, device=x.device)
    _rt._launch("split_f16_kernel", 0.0, 8.0 * rows * cols, _rt.lib().ispk_split_f16, x2.data_ptr(), x2.stride(0), out[0].data_ptr(),
                out[1].data_ptr(), cols, rows, cols, _rt._stream())
    return out


def layernorm_split(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], ada_scale: Optional[Tensor] = None,
                    ada_shift: Optional[Tensor] = None, rows_per_batch: int = 1, row_mask: Optional[Tensor] = None,
                    eps: float = 1e-5) -> Tensor:
    """ispk_layernorm_f32_split: `layernorm` with the result as split planes fp16 [2, ..., D]."""
    _rt._dev(x, gamma, beta, ada_scale, ada_shift, row_mask)
    assert x.dtype == torch.float32
    x2 = _rt._rows2d(x)
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
        row_mask = _rt._mask1d(row_mask)
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    label = f"layernorm_vec_kernel<{D // 128},split>" if D % 128 == 0 and D <= 512 else f"layernorm_kernel<{D // 64},split>"
    _rt._launch(label, 0.0, float(rows) * D * 8, _rt.lib().ispk_layernorm_f32_split, x2.data_ptr(), x2.stride(0), _rt._ptr(gamma),
                _rt._ptr(beta), _rt._ptr(ada_scale), _rt._ptr(ada_shift), ada_stride, rows_per_batch, _rt._ptr(row_mask), y.data_ptr(), D,
                y.stride(0), rows, D, eps, _rt._stream())
    return y


def _split_label(M: int, N: int, K: int) -> str:
    t = _rt.lib().ispk_gemm_split_f16_tile(M, N, K)
    return f"gemm_split_f16_kernel<{t // 100},{t // 10 % 10},{t % 10}>"


def gemm_split(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
               mask: Optional[Tensor] = None, flags: int = 0, out_split: bool = False) -> Tensor:
    """ispk_gemm_split_f16: epilogue(a @ w^T) with a = split planes [2, ..., K], w = split planes [2, N, K].
    Returns fp32 [..., N], or split planes [2, ..., N] with `out_split` (no residual)."""
    _rt._dev(a, w, bias, resid, mask)
    assert a.dtype == torch.float16 and w.dtype == torch.float16 and a.shape[0] == 2 and w.ndim == 3 and w.shape[0] == 2
    assert a.is_contiguous() and w.is_contiguous()
    K, N = a.shape[-1], w.shape[1]
    assert w.shape[2] == K
    M = a[0].numel() // K
    lead = a.shape[1:-1]
    r2 = None
    if resid is not None:
        r2 = _rt._rows2d(resid)
        assert r2.shape == (M, N) and r2.dtype == torch.float32 and not out_split
    if mask is not None:
        mask = _rt._mask1d(mask)
        assert mask.dtype == torch.bool
    if out_split:
        out = torch.empty((2, *lead, N), dtype=torch.float16, device=a.device)
        flags |= _rt.EP_OUT_SPLIT
        c_plane, nb_out = out.stride(0), 4.0 * M * N
    else:
        out = torch.empty((*lead, N), dtype=torch.float32, device=a.device)
        c_plane, nb_out = 0, 4.0 * M * N
    nb = 4.0 * M * K + 4.0 * N * K + nb_out + (4.0 * M * N if r2 is not None else 0.0)
    _rt._launch(_split_label(M, N, K), 2.0 * M * N * K, nb, _rt.lib().ispk_gemm_split_f16, a.data_ptr(), K, a.stride(0), w.data_ptr(), K,
                w.stride(0), out.data_ptr(), N, c_plane, _rt._ptr(bias), _rt._ptr(r2), _rt._ld(r2), _rt._ptr(mask), M, N,
                K, flags, 0, 0, _rt._stream())
    return out


def to_mel_split(dec: Tensor, w: Tensor, bias: Tensor, mask: Optional[Tensor]) -> Tensor:
    """mel[B, C, T] = mask * (dec @ w^T + bias) from split planes dec [2, B, T, D], w [2, C, D] (ISPK_EP_ROWS_T)."""
    _rt._dev(dec, w, bias, mask)
    _, B, T, D = dec.shape
    C = w.shape[1]
    out = torch.empty((B, C, T), dtype=torch.float32, device=dec.device)
    flags = _rt.EP_ROWS_T
    if mask is not None:
        mask = _rt._mask1d(mask)
        flags |= _rt.EP_MASK_OUT
    _rt._launch(_split_label(B * T, C, D), 2.0 * C * B * T * D, 4.0 * (B * T * D + C * D + B * C * T), _rt.lib().ispk_gemm_split_f16,
                dec.data_ptr(), D, dec.stride(0), w.data_ptr(), D, w.stride(0), out.data_ptr(), T, 0, _rt._ptr(bias), None, 0, _rt._ptr(mask),
                B * T, C, D, flags, T, C * T, _rt._stream())
    return out


def conv5_padded_split(xpad: Tensor, w2d: Tensor, flags: int = 0) -> Tensor:
    """`conv5_padded` on split planes: xpad [2, B, T+4, C], w2d [2, O, k*C] -> fp32 [B, T+4, O] (row t = frame t)."""
    _rt._dev(xpad, w2d)
    _, B, TP, C = xpad.shape
    _, O, K = w2d.shape
    taps = K // C
    assert taps * C == K and taps in (1, 5) and xpad.is_contiguous() and w2d.is_contiguous()
    out = torch.empty((B, TP, O), dtype=torch.float32, device=xpad.device)
    a_ptr = xpad.data_ptr() + (0 if taps == 5 else 2 * C * 2)   # k=1: frame t sits at padded row t+2
    M = B * TP - 4
    _rt._launch(_split_label(M, O, K), 2.0 * M * O * K, 4.0 * (M * C + O * K + M * O), _rt.lib().ispk_gemm_split_f16, a_ptr, C,
                xpad.stride(0), w2d.data_ptr(), K, w2d.stride(0), out.data_ptr(), O, 0, None, None, 0, None, M, O, K, flags, 0, 0,
                _rt._stream())
    return out


def alibi_mqa_attention_split(qkv: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor], out_split: bool = True) -> Tensor:
    """ispk_alibi_mqa_attn_split_f16: qkv fp32 [B, N, H*64 + 128] -> merged heads as split planes [2, B, N, H*64] (or fp32)."""
    _rt._dev(qkv, slopes, key_len)
    B, N, W = qkv.shape
    assert W == heads * 64 + 128 and qkv.is_contiguous() and qkv.dtype == torch.float32
    key_len = _rt._i64(key_len)
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
    _rt._launch("attn_split_f16_kernel", 256.0 * B * N * N * heads, float(B) * N * (2 * heads * 64 + 128) * 4,
                _rt.lib().ispk_alibi_mqa_attn_split_f16, qkv.data_ptr(), W, qkv.data_ptr() + heads * 64 * es,
                qkv.data_ptr() + (heads * 64 + 64) * es, W, slopes.data_ptr(), _rt._ptr(key_len), out.data_ptr(), heads * 64, plane, B, N,
                heads, _rt._stream())
    return out
