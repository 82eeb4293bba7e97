"""The training step (csrc/backward.hip, aligner_bwd.hip, attention_train.hip, train.hip): backward, losses, optimiser."""
import ctypes
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["transpose", "_TN_WORKSPACE_FLOATS", "_workspaces", "drop_workspace", "workspace", "gemm_tn", "gemm_gelu_train",
           "gemm_gelu_bwd", "gemm_tn_batched", "aligner_scores_bwd", "masked_instnorm_bwd", "soft_average_bwd", "layernorm_bwd",
           "gelu", "dropout_mask", "alibi_mqa_attention_train", "gelu_bwd", "alibi_mqa_attention_bwd", "mel_loss",
           "flow_loss_bwd", "adaln_bwd", "time_embedding_bwd", "attn_ctc_loss", "attn_bin_loss", "mel_grad_rows", "colsum",
           "smallk_wgrad", "embedding_bwd", "grad_sqnorm", "set_seed_source", "adam_args", "adamw_dev", "adamw"]


def transpose(x: Tensor) -> Tensor:
    """ispk_transpose_f32: y[c, r] = x[r, c] (fp32 matrix; weights for dX = dY . W through the NT GEMM)."""
    _rt._dev(x)
    assert x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1
    y = torch.empty((x.shape[1], x.shape[0]), dtype=torch.float32, device=x.device)
    _rt._launch("transpose_kernel", 0.0, 8.0 * x.numel(), _rt.lib().ispk_transpose_f32, x.data_ptr(), x.stride(0), y.data_ptr(),
                y.stride(0), x.shape[0], x.shape[1], _rt._stream())
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
    _rt._dev(a, b, row_mask, out)
    a2, b2 = _rt._rows2d(a), _rt._rows2d(b)
    in16 = a2.dtype == torch.bfloat16
    assert a2.dtype == b2.dtype and a2.dtype in (torch.float32, torch.bfloat16) and a2.shape[0] == b2.shape[0]
    M, N1 = a2.shape
    N2 = b2.shape[1]
    if out is None:
        assert not accumulate
        out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
    assert out.shape == (N1, N2) and out.stride(1) == 1 and out.dtype == torch.float32
    if row_mask is not None:
        row_mask = _rt._mask1d(row_mask)
        assert row_mask.dtype == torch.bool and row_mask.numel() == M
    if M == 0:      # a sum over no rows (the C entry refuses M = 0 and the NULL data_ptr() of an empty tensor)
        return out if accumulate else _rt._zero_rows(out)
    ws = _rt.workspace(a.device, N1 * N2)
    # one row: the leading dimensions are never stepped, and torch reports a single row's stride as its width whatever the
    # view's real stride was (reshape), which the bf16 entry refuses for N % 8 == 4 - pass a width the ABI accepts
    lda, ldb = (a2.stride(0), b2.stride(0)) if M > 1 else (-(-N1 // 8) * 8, -(-N2 // 8) * 8)
    fn = _rt.lib().ispk_gemm_tn_b16 if in16 else (_rt.lib().ispk_gemm_tn_bf16 if bf16 else _rt.lib().ispk_gemm_tn_f32)
    _rt._launch(f"gemm_tn_{'b16_' if in16 else ('bf16_' if bf16 else '')}kernel<{N1}x{N2}>", 2.0 * M * N1 * N2,
                float(a2.element_size()) * (a2.numel() + b2.numel()) + 4.0 * out.numel(), fn, a2.data_ptr(), lda, b2.data_ptr(), ldb,
                out.data_ptr(), out.stride(0), M, N1, N2, _rt._ptr(row_mask), int(accumulate), ws.data_ptr(), ws.numel(), _rt._stream())
    return out


def gemm_gelu_train(x: Tensor, w: Tensor, dropout_p: float = 0.0, seed: int = 0):
    """ispk_gemm_bf16_gelu_train -> (u, a): u = x @ w^T and a = dropout(gelu(u)), both bf16, from ONE launch (the first Linear
    of a feed-forward block in an AMP training step: `gemm(x, w)` followed by `gelu(u, dropout_p, seed)`, bit for bit).
    x bf16 [..., K], w bf16 [N, K], K = 256 / 384."""
    _rt._dev(x, w)
    x2 = _rt._rows2d(x)
    M, K = x2.shape
    N = w.shape[0]
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.shape[1] == K and w.stride(1) == 1
    u = torch.empty((*x.shape[:-1], N), dtype=torch.bfloat16, device=x.device)
    a = torch.empty_like(u)
    _rt._launch(f"gemm_bf16_panel_kernel<{K // 64},gelu_train>", 2.0 * M * N * K, 2.0 * (M * K + N * K + 2 * M * N), _rt.lib().ispk_gemm_bf16_gelu_train,
                x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), u.data_ptr(), N, a.data_ptr(), N, M, N, K, dropout_p,
                seed & 0xFFFFFFFFFFFFFFFF, _rt._stream())
    return u, a


def gemm_gelu_bwd(dy: Tensor, w2_t: Tensor, u: Tensor, mask: Optional[Tensor] = None, dropout_p: float = 0.0, seed: int = 0) -> Tensor:
    """ispk_gemm_bf16_gelu_bwd -> du = (mask dy @ w2_t^T) * gelu'(u) * [keep / (1 - p)] (bf16): the feed-forward backward's
    `gemm(dy, w2_t, mask=mask, flags=EP_MASK_OUT)` + `gelu_bwd(da, u, dropout_p=, seed=)` as ONE launch, bit for bit.
    dy bf16 [..., K], w2_t bf16 [N, K] (= W2^T rows), u bf16 [..., N]."""
    _rt._dev(dy, w2_t, u, mask)
    d2, u2 = _rt._rows2d(dy), _rt._rows2d(u)
    M, K = d2.shape
    N = w2_t.shape[0]
    assert dy.dtype == torch.bfloat16 and w2_t.dtype == torch.bfloat16 and u.dtype == torch.bfloat16 and u2.shape == (M, N) and u2.is_contiguous()
    if mask is not None:
        mask = _rt._mask1d(mask)
        assert mask.dtype == torch.bool and mask.numel() == M
    du = torch.empty_like(u)
    _rt._launch(f"gemm_bf16_panel_kernel<{K // 64},gelu_bwd>", 2.0 * M * N * K, 2.0 * (M * K + N * K + 2 * M * N), _rt.lib().ispk_gemm_bf16_gelu_bwd,
                d2.data_ptr(), d2.stride(0), w2_t.data_ptr(), w2_t.stride(0), u2.data_ptr(), N, du.data_ptr(), N, _rt._ptr(mask), M, N, K,
                dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _rt._stream())
    return du


def gemm_tn_batched(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ispk_gemm_tn_batched_f32: C[i] = a[i]^T b[i] for a [batch, M, N1], b [batch, M, N2] (fp32; any batch / row strides,
    unit column stride) -> [batch, N1, N2] (`out`: a view with the same freedom)."""
    _rt._dev(a, b, out)
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
        return out if batch == 0 else _rt._zero_rows(out)
    ws = _rt.workspace(a.device, batch * N1 * N2)
    _rt._launch("gemm_tn_kernel<batched>", 2.0 * batch * M * N1 * N2, 4.0 * (a.numel() + b.numel() + out.numel()),
                _rt.lib().ispk_gemm_tn_batched_f32, a.data_ptr(), a.stride(1), a.stride(0), b.data_ptr(), b.stride(1), b.stride(0),
                out.data_ptr(), out.stride(1), out.stride(0), batch, M, N1, N2, None, 0, ws.data_ptr(), ws.numel(), _rt._stream())
    return out


def aligner_scores_bwd(attn_logits: Tensor, attn_soft: Tensor, d_soft: Optional[Tensor], d_logits: Optional[Tensor],
                       text_len: Tensor, mel_len: Tensor, scale: float):
    """ispk_aligner_scores_bwd_f32 -> (dS [B, M, L4], dSt [B, L, M4]) zero-padded to multiples of 4 columns."""
    _rt._dev(attn_logits, attn_soft, d_soft, d_logits, text_len, mel_len)
    B, M, L = attn_logits.shape
    L4, M4 = (L + 3) // 4 * 4, (M + 3) // 4 * 4
    dS = _rt.zeros((B, M, L4), torch.float32, attn_logits.device)
    dSt = _rt.zeros((B, L, M4), torch.float32, attn_logits.device)
    cg = lambda t: None if t is None else t.float().contiguous()       # noqa: E731
    d_soft, d_logits = cg(d_soft), cg(d_logits)
    _rt._launch("aligner_scores_bwd_kernel", 0.0, 4.0 * B * M * L * 6, _rt.lib().ispk_aligner_scores_bwd_f32, attn_logits.contiguous().data_ptr(),
                attn_soft.contiguous().data_ptr(), _rt._ptr(d_soft), _rt._ptr(d_logits), _rt._i64(text_len).data_ptr(),
                _rt._i64(mel_len).data_ptr(), dS.data_ptr(), L4, dSt.data_ptr(), M4, B, M, L, scale, _rt._stream())
    return dS, dSt


def masked_instnorm_bwd(y: Tensor, d_out: Tensor, weight: Tensor, lengths: Tensor, eps: float = 1e-5):
    """ispk_masked_instnorm_bwd_f32: y, d_out [B, T+4, C] (row t = frame t) -> (d_y like y, d_weight [C], d_bias [C])."""
    _rt._dev(y, d_out, weight, lengths)
    B, TP, C = y.shape
    assert y.is_contiguous() and d_out.is_contiguous() and d_out.shape == y.shape and y.dtype == torch.float32
    d_y = torch.empty_like(y)
    dw, db = torch.empty((C,), dtype=torch.float32, device=y.device), torch.empty((C,), dtype=torch.float32, device=y.device)
    ws = _rt.workspace(y.device, 2 * B * C)
    _rt._launch("masked_instnorm_bwd_kernel", 0.0, 4.0 * y.numel() * 5, _rt.lib().ispk_masked_instnorm_bwd_f32, y.data_ptr(), d_out.data_ptr(),
                weight.data_ptr(), _rt._i64(lengths).data_ptr(), d_y.data_ptr(), dw.data_ptr(), db.data_ptr(),
                ws.data_ptr(), ws.numel(), B, TP - 4, C, eps, _rt._stream())
    return d_y, dw, db


def soft_average_bwd(attn_soft: Tensor, pitch: Tensor, energy: Tensor, d_feats: Tensor, text_len: Tensor,
                     out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """ispk_soft_average_bwd_f32 -> d attn_soft [B, M, L].  `out`: written in place (contiguous fp32 [B, M, L]); with `accumulate`
    the gradient is added to what `out` holds."""
    _rt._dev(attn_soft, pitch, energy, d_feats, text_len, out)
    B, M, L = attn_soft.shape
    if out is None:
        assert not accumulate, "soft_average_bwd: accumulate needs `out`"
        d = torch.empty_like(attn_soft)
    else:
        assert out.shape == (B, M, L) and out.dtype == torch.float32 and out.is_contiguous()
        d = out
    ws = _rt.workspace(attn_soft.device, 3 * B * L)
    _rt._launch("soft_average_bwd_kernels", 0.0, 4.0 * attn_soft.numel() * 3, _rt.lib().ispk_soft_average_bwd_f32,
                attn_soft.contiguous().data_ptr(), pitch.float().contiguous().data_ptr(), energy.float().contiguous().data_ptr(),
                d_feats.float().contiguous().data_ptr(), _rt._i64(text_len).data_ptr(), ws.data_ptr(), ws.numel(),
                d.data_ptr(), int(bool(accumulate)), B, M, L, _rt._stream())
    return d


def layernorm_bwd(x: Tensor, dy: Tensor, gamma: Optional[Tensor], row_mask: Optional[Tensor] = None,
                  dx: Optional[Tensor] = None, add_to_dx: bool = False, want_param_grads: bool = True, eps: float = 1e-5,
                  bf16_copy: bool = False):
    """ispk_layernorm_bwd_f32 -> (dx, dgamma | None, dbeta | None).  `dx` given + add_to_dx: accumulated in place (the
    residual branch's gradient is already there).  `bf16_copy` (ispk_layernorm_bwd_dual_f32): a fourth result, dx once more
    as bf16 rows - the operand an AMP step's next dX GEMM and weight gradient take, without a cast launch."""
    _rt._dev(x, dy, gamma, row_mask, dx)
    x2, dy2 = _rt._rows2d(x), _rt._rows2d(dy)
    rows, D = x2.shape
    assert x2.dtype == torch.float32 and dy2.dtype == torch.float32 and dy2.shape == x2.shape
    if dx is None:
        assert not add_to_dx
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dx2 = _rt._rows2d(dx)
    if row_mask is not None:
        row_mask = _rt._mask1d(row_mask)
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    dg = db = None
    ws = None
    if want_param_grads:
        dg = torch.empty((D,), dtype=torch.float32, device=x.device)
        db = torch.empty((D,), dtype=torch.float32, device=x.device)
        ws = _rt.workspace(x.device, ((rows + 63) // 64) * 2 * D)
    if bf16_copy:
        dx16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        _rt._launch(f"layernorm_bwd_kernel<{D // 64}>", 0.0, 4.0 * rows * D * (3.5 + int(add_to_dx)), _rt.lib().ispk_layernorm_bwd_dual_f32,
                    x2.data_ptr(), x2.stride(0), dy2.data_ptr(), dy2.stride(0), _rt._ptr(gamma), _rt._ptr(row_mask), dx2.data_ptr(),
                    dx2.stride(0), int(add_to_dx), _rt._ptr(dg), _rt._ptr(db), _rt._ptr(ws), ws.numel() if ws is not None else 0, rows, D, eps,
                    dx16.data_ptr(), D, _rt._stream())
        return dx, dg, db, dx16
    _rt._launch(f"layernorm_bwd_kernel<{D // 64}>", 0.0, 4.0 * rows * D * (3 + int(add_to_dx)), _rt.lib().ispk_layernorm_bwd_f32,
                x2.data_ptr(), x2.stride(0), dy2.data_ptr(), dy2.stride(0), _rt._ptr(gamma), _rt._ptr(row_mask), dx2.data_ptr(),
                dx2.stride(0), int(add_to_dx), _rt._ptr(dg), _rt._ptr(db), _rt._ptr(ws), ws.numel() if ws is not None else 0, rows, D, eps,
                _rt._stream())
    return dx, dg, db


def gelu(u: Tensor, dropout_p: float = 0.0, seed: int = 0, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_gelu_f32 / ispk_gelu_f32_bf16: exact-erf GELU as its own pass (the training forward keeps u), optionally followed
    by dropout; `out_dtype=torch.bfloat16`: the result as the bf16 operand an AMP step's second Linear takes."""
    _rt._dev(u)
    assert u.dtype in (torch.float32, torch.bfloat16) and u.is_contiguous() and out_dtype in (torch.float32, torch.bfloat16)
    if u.dtype == torch.bfloat16:      # ispk_gelu_bf16: the pre-activation itself is bf16 (autocast's Linear output)
        assert out_dtype == torch.bfloat16
        fn = _rt.lib().ispk_gelu_bf16
    else:
        fn = _rt.lib().ispk_gelu_f32 if out_dtype == torch.float32 else _rt.lib().ispk_gelu_f32_bf16
    a = torch.empty(u.shape, dtype=out_dtype, device=u.device)
    _rt._launch("gelu_fwd_kernel", 0.0, float(u.element_size() + a.element_size()) * u.numel(), fn, u.data_ptr(), a.data_ptr(), u.numel(),
                dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _rt._stream())
    return a


def dropout_mask(n: int, dropout_p: float, seed: int, device) -> Tensor:
    """ispk_dropout_mask_u8: the keep mask the kernels evaluate for element indices 0 .. n-1 (bool [n])."""
    out = torch.empty((n,), dtype=torch.bool, device=device)
    _rt._dev(out)
    _rt._check(_rt.lib().ispk_dropout_mask_u8(out.data_ptr(), n, dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _rt._stream()), "ispk_dropout_mask_u8")
    return out


def alibi_mqa_attention_train(qkv: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor], dropout_p: float, seed: int):
    """-> (o [B, N, heads*64] in qkv's dtype, lse fp32 [B, heads, N]): attention with dropped probabilities, row statistics
    kept for the backward.  fp32 qkv: ispk_alibi_mqa_attn_train_f32.  bf16 qkv (the step under autocast):
    ispk_alibi_mqa_attn_train_bf16 - bf16 MFMAs, K / V staged in LDS, bf16 o."""
    _rt._dev(qkv, slopes, key_len)
    B, N, W = qkv.shape
    b16 = qkv.dtype == torch.bfloat16
    assert W == heads * 64 + 128 and qkv.dtype in (torch.float32, torch.bfloat16) and qkv.is_contiguous()
    slopes = slopes.to(torch.float32).contiguous()
    key_len = _rt._i64(key_len)
    o = torch.empty((B, N, heads * 64), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see alibi_mqa_attention_raw)
        return o, lse
    _rt._launch("attn_train_fwd_bf16_kernel" if b16 else "attn_train_fwd_kernel", 4.0 * B * heads * N * N * 64,
                float(qkv.element_size()) * (qkv.numel() + o.numel()),
                _rt.lib().ispk_alibi_mqa_attn_train_bf16 if b16 else _rt.lib().ispk_alibi_mqa_attn_train_f32, qkv.data_ptr(), W, slopes.data_ptr(),
                _rt._ptr(key_len), o.data_ptr(), heads * 64, lse.data_ptr(), B, N, heads, dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _rt._stream())
    return o, lse


def gelu_bwd(da: Tensor, u: Tensor, out: Optional[Tensor] = None, dropout_p: float = 0.0, seed: int = 0) -> Tensor:
    """ispk_gelu_bwd_f32: du = da * [keep / (1 - p)] * gelu'(u) (exact erf); `out` may alias `da`."""
    _rt._dev(da, u, out)
    assert da.dtype in (torch.float32, torch.bfloat16) and u.dtype in (torch.float32, torch.bfloat16) and da.is_contiguous() and u.is_contiguous()
    assert da.shape == u.shape and (u.dtype == torch.float32 or da.dtype == torch.bfloat16)
    if out is None:
        out = torch.empty_like(da)
    assert out.dtype == da.dtype
    b16 = da.dtype == torch.bfloat16      # ispk_gelu_bwd_bf16: da and du are bf16 GEMM operands of an AMP step (_b16: u bf16 too)
    fn = (_rt.lib().ispk_gelu_bwd_b16 if u.dtype == torch.bfloat16 else _rt.lib().ispk_gelu_bwd_bf16) if b16 else _rt.lib().ispk_gelu_bwd_f32
    _rt._launch("gelu_bwd_kernel", 0.0, float(u.element_size() + 2 * da.element_size()) * da.numel(), fn,
                da.data_ptr(), u.data_ptr(), out.data_ptr(), da.numel(), dropout_p, seed & 0xFFFFFFFFFFFFFFFF, _rt._stream())
    return out


def alibi_mqa_attention_bwd(qkv: Tensor, o: Tensor, d_o: Tensor, heads: int, slopes: Tensor, key_len: Optional[Tensor],
                            lse: Optional[Tensor] = None, dropout_p: float = 0.0, seed: int = 0):
    """-> (dqkv like qkv, dlogslopes fp32 [heads]).  fp32 tensors: ispk_alibi_mqa_attn_bwd_f32 (`lse` from the training
    forward saves the statistics pass).  bf16 tensors (the step under autocast): ispk_alibi_mqa_attn_bwd_bf16, `lse` required.
    dropout_p / seed must be the forward's."""
    _rt._dev(qkv, o, d_o, slopes, key_len, lse)
    B, N, W = qkv.shape
    b16 = qkv.dtype == torch.bfloat16
    assert W == heads * 64 + 128 and qkv.dtype in (torch.float32, torch.bfloat16) and qkv.is_contiguous()
    assert o.shape == (B, N, heads * 64) and d_o.shape == o.shape and o.dtype == qkv.dtype and d_o.dtype == qkv.dtype
    o, d_o = o.contiguous(), d_o.contiguous()
    slopes = slopes.to(torch.float32).contiguous()
    key_len = _rt._i64(key_len)
    dqkv = torch.empty_like(qkv)
    dls = torch.empty((heads,), dtype=torch.float32, device=qkv.device)
    if B == 0:      # no rows, no gradient (NULL data_ptr() of an empty tensor: see alibi_mqa_attention_raw)
        return dqkv, dls.zero_()
    if b16:
        assert lse is not None and lse.dtype == torch.float32 and lse.shape == (B, heads, N) and lse.is_contiguous()
        ws = _rt.workspace(qkv.device, B * heads * N + 2 * heads * B * ((N + 63) // 64))
        _rt._launch("attn_bwd_bf16_kernels", 10.0 * B * heads * N * N * 64, 2.0 * (2 * qkv.numel() + 2 * o.numel()),
                    _rt.lib().ispk_alibi_mqa_attn_bwd_bf16, qkv.data_ptr(), W, o.data_ptr(), d_o.data_ptr(), heads * 64, slopes.data_ptr(),
                    _rt._ptr(key_len), lse.data_ptr(), dqkv.data_ptr(), dls.data_ptr(), ws.data_ptr(), ws.numel(), B, N, heads, dropout_p,
                    seed & 0xFFFFFFFFFFFFFFFF, _rt._stream())
        return dqkv, dls
    tiles = (N + 31) // 32
    ws = _rt.workspace(qkv.device, 2 * B * heads * N + heads * B * tiles)
    _rt._launch("attn_bwd_kernels", 10.0 * B * heads * N * N * 64, 4.0 * (2 * qkv.numel() + 2 * o.numel()),
                _rt.lib().ispk_alibi_mqa_attn_bwd_f32, qkv.data_ptr(), W, o.data_ptr(), d_o.data_ptr(), heads * 64, slopes.data_ptr(),
                _rt._ptr(key_len), dqkv.data_ptr(), dls.data_ptr(), ws.data_ptr(), ws.numel(), B, N, heads, _rt._ptr(lse), dropout_p,
                seed & 0xFFFFFFFFFFFFFFFF, _rt._stream())
    return dqkv, dls


def mel_loss(mel_out: Tensor, mel_target: Tensor, mel_len: Tensor, want_grad: bool = False, grad_out: float = 1.0):
    """ispk_mel_loss_f32 -> (loss fp32 [1], grad fp32 like mel_out | None)."""
    _rt._dev(mel_out, mel_target, mel_len)
    assert mel_out.dtype == torch.float32 and mel_target.dtype == torch.float32 and mel_out.shape == mel_target.shape
    mel_out, mel_target = mel_out.contiguous(), mel_target.contiguous()
    B, C, T = mel_out.shape
    mel_len = _rt._i64(mel_len)
    ratio = torch.empty((B,), dtype=torch.float32, device=mel_out.device)
    loss = torch.empty((1,), dtype=torch.float32, device=mel_out.device)
    grad = torch.empty_like(mel_out) if want_grad else None
    _rt._launch("mel_loss_kernel", 0.0, 4.0 * mel_out.numel() * (2 + int(want_grad)), _rt.lib().ispk_mel_loss_f32, mel_out.data_ptr(),
                mel_target.data_ptr(), mel_len.data_ptr(), ratio.data_ptr(), loss.data_ptr(), _rt._ptr(grad), grad_out, B, C, T,
                _rt._stream())
    return loss, grad


def flow_loss_bwd(pred_raw: Tensor, flow: Tensor, mask: Tensor, grad_out: float = 1.0) -> Tensor:
    """ispk_flow_loss_bwd_f32: gradient of the flow loss wrt the predictor's raw output [B, L, C]."""
    _rt._dev(pred_raw, flow, mask)
    pred_raw, flow, mask = pred_raw.contiguous(), flow.contiguous(), mask.contiguous()
    B, L, C = pred_raw.shape
    assert mask.dtype == torch.bool and mask.shape == (B, L) and flow.shape == pred_raw.shape
    d = torch.empty_like(pred_raw)
    _rt._launch("flow_loss_bwd_kernel", 0.0, 12.0 * pred_raw.numel(), _rt.lib().ispk_flow_loss_bwd_f32, pred_raw.data_ptr(), flow.data_ptr(),
                mask.data_ptr(), grad_out, d.data_ptr(), B, L, C, _rt._stream())
    return d


def adaln_bwd(x: Tensor, dy: Tensor, scale: Tensor, row_mask: Optional[Tensor], dx: Optional[Tensor], add_to_dx: bool,
              dscale: Tensor, dshift: Tensor, eps: float = 1e-5) -> Tensor:
    """ispk_adaln_bwd_f32: x, dy [B, L, D]; scale / dscale / dshift [B, D] rows (any row stride, unit column stride)."""
    _rt._dev(x, dy, scale, row_mask, dx, dscale, dshift)
    B, L, D = x.shape
    x2, dy2 = _rt._rows2d(x), _rt._rows2d(dy)
    if dx is None:
        assert not add_to_dx
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dx2 = _rt._rows2d(dx)
    row_mask = _rt._mask1d(row_mask)
    assert scale.stride(1) == 1 and dscale.stride(1) == 1 and dshift.stride(1) == 1 and dscale.stride(0) == dshift.stride(0)
    _rt._launch(f"adaln_bwd_kernel<{D // 64}>", 0.0, 4.0 * x2.numel() * (3 + int(add_to_dx)), _rt.lib().ispk_adaln_bwd_f32, x2.data_ptr(),
                x2.stride(0), dy2.data_ptr(), dy2.stride(0), scale.data_ptr(), scale.stride(0), _rt._ptr(row_mask), dx2.data_ptr(),
                dx2.stride(0), int(add_to_dx), dscale.data_ptr(), dshift.data_ptr(), dscale.stride(0), B, L, D, eps, _rt._stream())
    return dx


def time_embedding_bwd(t: Tensor, inv_freq: Tensor, freq_scale: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, d_out: Tensor):
    """ispk_time_embedding_bwd_f32 -> (dw0, db0, dw1, db1)."""
    _rt._dev(t, inv_freq, freq_scale, w0, b0, w1, d_out)
    t = t.reshape(-1).float().contiguous()
    d_out = d_out.reshape(t.numel(), -1).float().contiguous()
    E, H = w1.shape[0], inv_freq.numel()
    dw0, db0 = torch.empty_like(w0, dtype=torch.float32), torch.empty((E,), dtype=torch.float32, device=t.device)
    dw1, db1 = torch.empty((E, E), dtype=torch.float32, device=t.device), torch.empty((E,), dtype=torch.float32, device=t.device)
    _rt._launch("time_embedding_bwd_kernel", 0.0, 0.0, _rt.lib().ispk_time_embedding_bwd_f32, t.data_ptr(), t.numel(),
                inv_freq.contiguous().data_ptr(), freq_scale.data_ptr(), H, w0.contiguous().data_ptr(), b0.data_ptr(),
                w1.contiguous().data_ptr(), E, d_out.data_ptr(), dw0.data_ptr(), db0.data_ptr(), dw1.data_ptr(), db1.data_ptr(), _rt._stream())
    return dw0, db0, dw1, db1


def attn_ctc_loss(attn_logits: Tensor, text_len: Tensor, mel_len: Tensor, blank_logprob: float = -1.0,
                  want_grad: bool = False, grad_out: float = 1.0):
    """ispk_attn_ctc_loss_f32 -> (loss fp32 [1], grad fp32 like attn_logits | None)."""
    _rt._dev(attn_logits, text_len, mel_len)
    assert attn_logits.dtype == torch.float32
    lg = attn_logits.reshape(-1, *attn_logits.shape[-2:]).contiguous()
    B, M, L = lg.shape
    text_len, mel_len = _rt._i64(text_len), _rt._i64(mel_len)
    s_pad = (2 * L + 1 + 63) // 64 * 64
    ws = _rt.workspace(lg.device, B * M + B + 2 * B * M * s_pad)
    loss = torch.empty((1,), dtype=torch.float32, device=lg.device)
    grad = torch.empty_like(lg) if want_grad else None
    _rt._launch("ctc_loss_kernels", 0.0, 4.0 * (lg.numel() * (2 + int(want_grad)) + 4 * B * M * s_pad), _rt.lib().ispk_attn_ctc_loss_f32,
                lg.data_ptr(), text_len.data_ptr(), mel_len.data_ptr(), blank_logprob, ws.data_ptr(), ws.numel(), loss.data_ptr(),
                _rt._ptr(grad), grad_out, B, M, L, _rt._stream())
    return loss, (grad.view(attn_logits.shape) if grad is not None else None)


def attn_bin_loss(attn_soft: Tensor, attn_hard: Tensor, eps: float = 1e-6, want_grad: bool = False, grad_out: float = 1.0):
    """ispk_attn_bin_loss_f32 -> (loss fp32 [2] = (loss, number of path cells), grad fp32 like attn_soft | None)."""
    _rt._dev(attn_soft, attn_hard)
    assert attn_soft.dtype == torch.float32 and attn_hard.dtype == torch.int16 and attn_soft.shape == attn_hard.shape
    attn_soft, attn_hard = attn_soft.contiguous(), attn_hard.contiguous()
    B, M, L = attn_soft.shape[0], attn_soft.shape[-2], attn_soft.shape[-1]
    loss = torch.empty((2,), dtype=torch.float32, device=attn_soft.device)
    grad = _rt.zeros(attn_soft.shape, attn_soft.dtype, attn_soft.device) if want_grad else None
    ws = _rt.workspace(attn_soft.device, 2048)
    _rt._launch("bin_loss_kernels", 0.0, 6.0 * attn_soft.numel(), _rt.lib().ispk_attn_bin_loss_f32, attn_soft.data_ptr(),
                attn_hard.data_ptr(), eps, ws.data_ptr(), loss.data_ptr(), _rt._ptr(grad), grad_out, B, M, L, _rt._stream())
    return loss, grad


def mel_grad_rows(dmel: Tensor, mask: Optional[Tensor]) -> Tensor:
    """ispk_mel_grad_rows_f32: [B, C, T] gradient of the mel output -> masked rows [B, T, C] for to_mel's backward."""
    _rt._dev(dmel, mask)
    assert dmel.dtype == torch.float32 and dmel.ndim == 3
    dmel = dmel.contiguous()
    B, C, T = dmel.shape
    if mask is not None:
        mask = mask.contiguous()
        assert mask.dtype == torch.bool and mask.shape == (B, T)
    g = torch.empty((B, T, C), dtype=torch.float32, device=dmel.device)
    _rt._launch("mel_grad_rows_kernel", 0.0, 8.0 * dmel.numel(), _rt.lib().ispk_mel_grad_rows_f32, dmel.data_ptr(), _rt._ptr(mask),
                g.data_ptr(), B, C, T, _rt._stream())
    return g


def colsum(x: Tensor, row_mask: Optional[Tensor] = None) -> Tensor:
    """ispk_colsum_f32: column sums of a [rows, cols] fp32 matrix (bias gradients) over the rows `row_mask` keeps, fixed order."""
    _rt._dev(x, row_mask)
    x2 = _rt._rows2d(x)
    assert x2.dtype == torch.float32
    rows, cols = x2.shape
    if row_mask is not None:
        row_mask = _rt._mask1d(row_mask)
        assert row_mask.dtype == torch.bool and row_mask.numel() == rows
    out = torch.empty((cols,), dtype=torch.float32, device=x.device)
    if rows == 0:
        return _rt.zero_(out)
    ws = _rt.workspace(x.device, 256 * cols)
    _rt._launch("colsum_kernels", 0.0, 4.0 * x2.numel(), _rt.lib().ispk_colsum_f32, x2.data_ptr(), x2.stride(0), rows, cols,
                _rt._ptr(row_mask), ws.data_ptr(), ws.numel(), out.data_ptr(), _rt._stream())
    return out


def smallk_wgrad(g: Tensor, x: Tensor) -> Tensor:
    """ispk_smallk_wgrad_f32: out[n, k] = sum_r g[r, n] x[r, k] for a Linear with K <= 8 input features."""
    _rt._dev(g, x)
    g2, x2 = _rt._rows2d(g), _rt._rows2d(x)
    assert g2.dtype == torch.float32 and x2.dtype == torch.float32 and g2.shape[0] == x2.shape[0] and x2.shape[1] <= 8
    rows, N = g2.shape
    K = x2.shape[1]
    out = torch.empty((N, K), dtype=torch.float32, device=g.device)
    if rows == 0:
        return _rt.zero_(out)
    ws = _rt.workspace(g.device, 256 * N * K)
    _rt._launch("smallk_wgrad_kernels", 2.0 * rows * N * K, 4.0 * (g2.numel() + x2.numel()), _rt.lib().ispk_smallk_wgrad_f32, g2.data_ptr(),
                g2.stride(0), x2.data_ptr(), x2.stride(0), rows, N, K, ws.data_ptr(), ws.numel(), out.data_ptr(), _rt._stream())
    return out


def embedding_bwd(ids: Tensor, d_emb: Tensor, vocab: int, padding_idx: int = 0) -> Tensor:
    """ispk_embedding_bwd_f32 -> d_table fp32 [vocab, D]."""
    _rt._dev(ids, d_emb)
    ids = ids.reshape(-1).to(torch.int64).contiguous()
    d2 = _rt._rows2d(d_emb).contiguous()
    assert d2.dtype == torch.float32 and d2.shape[0] == ids.numel()
    out = torch.empty((vocab, d2.shape[1]), dtype=torch.float32, device=d_emb.device)
    _rt._launch("embedding_bwd_kernel", 0.0, 4.0 * d2.numel(), _rt.lib().ispk_embedding_bwd_f32, ids.data_ptr(), d2.data_ptr(), ids.numel(),
                d2.shape[1], vocab, padding_idx, out.data_ptr(), out.stride(0), _rt._stream())
    return out


def grad_sqnorm(g: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ispk_grad_sqnorm_f32: sum of squares of a flat fp32 arena -> fp32 [1] (device)."""
    _rt._dev(g, out)
    assert g.dtype == torch.float32 and g.ndim == 1 and g.is_contiguous()
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=g.device)
    part = _rt.workspace(g.device, 2048)
    _rt._launch("sqnorm_kernels", 0.0, 4.0 * g.numel(), _rt.lib().ispk_grad_sqnorm_f32, g.data_ptr(), g.numel(), part.data_ptr(),
                out.data_ptr(), _rt._stream())
    return out


def set_seed_source(word: Optional[Tensor]) -> None:
    """ispk_set_dropout_seed_source: while set (a one-element int64 DEVICE tensor the caller keeps alive), every dropout kernel
    launched by this process - from the calling thread or from autograd's backward worker - folds that word into its seed
    when it runs: what lets a captured training step draw fresh masks on every replay.  None switches it off."""
    if word is not None:
        _rt._dev(word)
        assert word.dtype == torch.int64 and word.numel() == 1
    _rt._check(_rt.lib().ispk_set_dropout_seed_source(None if word is None else word.data_ptr()), "set_dropout_seed_source")


def adam_args(lr: float, betas: tuple, eps: float, weight_decay: float, step: int, max_norm: float = 1.0,
              grad_scale: float = 1.0) -> Tensor:
    """ispk_adam_args_f32 -> the 10 fp32 factors of AdamW step `step` as a pinned host tensor (for a copy to the device
    record that ispk_adamw_f32_dev reads)."""
    buf = (ctypes.c_float * 10)()
    _rt._check(_rt.lib().ispk_adam_args_f32(lr, betas[0], betas[1], eps, weight_decay, step, max_norm, grad_scale,
                                            ctypes.cast(buf, ctypes.c_void_p)), "adam_args")
    t = torch.tensor(list(buf), dtype=torch.float32)
    return t.pin_memory() if torch.cuda.is_available() else t


def adamw_dev(p: Tensor, g: Tensor, m: Tensor, v: Tensor, n_decay: int, args_dev: Tensor, grad_sqnorm: Optional[Tensor] = None) -> None:
    """ispk_adamw_f32_dev: `adamw` with the step's factors read from the device record `args_dev` (fp32 [10], adam_args)."""
    _rt._dev(p, g, m, v, args_dev, grad_sqnorm)
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.ndim == 1 and t.is_contiguous() and t.numel() == p.numel()
    assert args_dev.dtype == torch.float32 and args_dev.numel() == 10 and args_dev.is_contiguous()
    _rt._launch("adamw_kernel", 0.0, 28.0 * p.numel(), _rt.lib().ispk_adamw_f32_dev, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                p.numel(), n_decay, args_dev.data_ptr(), _rt._ptr(grad_sqnorm), _rt._stream())


def adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, n_decay: int, lr: float, betas: tuple, eps: float, weight_decay: float,
          step: int, grad_sqnorm: Optional[Tensor] = None, max_norm: float = 1.0, grad_scale: float = 1.0) -> None:
    """ispk_adamw_f32 over flat fp32 arenas (in place)."""
    _rt._dev(p, g, m, v, grad_sqnorm)
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.ndim == 1 and t.is_contiguous() and t.numel() == p.numel()
    _rt._launch("adamw_kernel", 0.0, 28.0 * p.numel(), _rt.lib().ispk_adamw_f32, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                p.numel(), n_decay, lr, betas[0], betas[1], eps, weight_decay, step, _rt._ptr(grad_sqnorm), max_norm, grad_scale,
                _rt._stream())
