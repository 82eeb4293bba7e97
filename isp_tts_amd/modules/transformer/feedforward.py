"""`FeedForward`: Linear -> GELU(erf) -> Linear (tts/modules/transformer/feedforward.py:20-40 of the reference).

Two MFMA GEMMs; the exact-erf GELU (layers.py:29) is the first GEMM's epilogue, and the second GEMM's epilogue can
carry the residual add and row mask of transformer.py:105,110.  Dropout is identity in eval (the forward path).
Inside a `TransformerLayer` the block runs in one of the fused forms below; which one is `plan.select_plan`'s decision.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from ... import runtime
from ...staging import StagedWeights
from ..constructor import Constructor, ModuleConfig
from . import plan
from .plan import Consumer, Form

_ACTS = {"gelu": runtime.EP_GELU, "swish": runtime.EP_SILU, "linear": 0}


@dataclass
class FeedForwardConfig(ModuleConfig):
    dim: int = 384
    inner_dim: int = 1536
    dropout: float = 0.0
    activation: str = "relu"
    bias: bool = False
    glu: bool = False


class FeedForward(nn.Module, Constructor):
    def __init__(self, dim: int = 384, inner_dim: int = 1536, dropout: float = 0.0, activation: str = "relu",
                 bias: bool = False, glu: bool = False):
        super().__init__()
        if glu or activation not in _ACTS:
            raise NotImplementedError(f"built for the recipes' feed-forward (gelu, no GLU); got activation="
                                      f"{activation!r}, glu={glu}")
        self.act_flag = _ACTS[activation]
        self.dropout_p = dropout
        # same container layout as the reference so the keys are net.0.weight / net.3.weight
        self.net = nn.Sequential(nn.Linear(dim, inner_dim, bias=bias), nn.GELU() if activation == "gelu" else nn.Identity(),
                                 nn.Dropout(dropout) if dropout > 0. else nn.Identity(),
                                 nn.Linear(inner_dim, dim, bias=bias))
        self.compute_dtype = torch.float32
        self._cache = StagedWeights()

    def _staged(self, dtype: torch.dtype):
        ps = (self.net[0].weight, self.net[3].weight)
        if dtype == torch.float16:   # split fp16 planes [2, N, K] for the split-fp16 kernels
            return self._cache.get(dtype, ps, lambda: (runtime.split_f16(ps[0].detach().float().contiguous()),
                                                       runtime.split_f16(ps[1].detach().float().contiguous())))
        if dtype == torch.bfloat16 and ps[0].is_cuda and ps[0].dtype == torch.float32:   # libispk launches (re-staged every training step)
            return self._cache.get(dtype, ps, lambda: (runtime.cast_bf16(ps[0].detach()), runtime.cast_bf16(ps[1].detach())))
        return self._cache.get(dtype, ps, lambda: (ps[0].detach().to(dtype).contiguous(),
                                                   ps[1].detach().to(dtype).contiguous()))

    def _packed_w2(self) -> Tensor:
        """W2 in the fused kernel's chunk-contiguous layout, staged once per weight version."""
        return self._cache.get("w2p", (self.net[3].weight,),
                               lambda: runtime.ffn_pack_w2(self._staged(torch.bfloat16)[1]))

    def _chunked_w2(self) -> Tensor:
        """W2 as chunk-contiguous [inner/32][D][32] blocks (ispk_ffn_bf16_prenorm2), staged once per weight version."""
        return self._cache.get("w2c", (self.net[3].weight,),
                               lambda: runtime.ffn_chunk_w2(self._staged(torch.bfloat16)[1]))

    # ---- the fused forms of a layer's second half (bf16 path, x fp32): one method each, no decisions ----

    def attn_out_ffn(self, x: Tensor, attn_out: Tensor, woc: Tensor, norm, mask: Optional[Tensor], form: Form,
                     consumer: Optional[Consumer] = None, store_out: bool = True):
        """x1 = x + [mask] * to_out(attn_out), y = [mask] * (x1 + feed_forward(norm(x1))) in one kernel (ispk_attn_out_ffn_bf16):
        x1 exists only in the kernel's accumulators.  x: the LAYER's input, `woc` = Attention._chunked_wo().  -> (y, second) with
        second by `form`: None, the output rows' (mean, rstd) for `consumer`, the q/kv rows of the layer `consumer` belongs to
        (bf16 [..., 512]), or LN_final(y) in `consumer.dtype` - then, without `store_out`, y itself is not stored (None)."""
        w1, _ = self._staged(torch.bfloat16)
        kw = {}
        if form is Form.ATTN_OUT_FFN_NORM:
            kw = dict(final_norm=(consumer.weight, consumer.bias, consumer.eps, consumer.apply_mask, consumer.dtype),
                      want_out=store_out)
        elif form is Form.ATTN_OUT_FFN_QKV:
            kw = dict(next_qkv=(consumer.weight, consumer.bias, consumer.eps, consumer.attention._chunked_wqkv()))
        elif form is Form.ATTN_OUT_FFN_STATS:
            kw = dict(want_stats=True, stats_eps=consumer.eps)
        res = runtime.attn_out_ffn(x, attn_out, woc, norm.weight, norm.bias, w1, self._chunked_w2(), mask=mask,
                                   norm_eps=norm.eps, **kw)
        return (res, None) if form is Form.ATTN_OUT_FFN else res

    def prenorm(self, x: Tensor, norm, mask: Optional[Tensor], pair: bool, stats_eps: Optional[float] = None):
        """(y, stats | None): y = [mask] * (x + feed_forward(norm(x))) in one kernel whose waves own whole rows - the eight-wave
        ispk_ffn_bf16_prenorm2 (`pair`, csrc/ffn2.hip) or the four-wave ispk_ffn_bf16_prenorm; with `stats_eps` also the output
        rows' (mean, rstd) for the next layer's q/kv GEMM.  The `* mask` of transformer.py:102 cannot reach a kept value
        because the same mask multiplies the block's output (:110)."""
        w1, _ = self._staged(torch.bfloat16)
        kw = dict(mask=mask, flags=runtime.EP_MASK_OUT if mask is not None else 0, norm_eps=norm.eps,
                  want_stats=stats_eps is not None, stats_eps=1e-5 if stats_eps is None else stats_eps)
        if pair:
            res = runtime.ffn_prenorm2(x, norm.weight, norm.bias, w1, self._chunked_w2(), **kw)
        else:
            res = runtime.ffn_prenorm(x, norm.weight, norm.bias, w1, self._packed_w2(), bias2=self.net[3].bias, **kw)
        return (res, None) if stats_eps is None else res

    def prenorm_split(self, x: Tensor, norm, mask: Optional[Tensor], splits: int, consumer: Optional[Consumer] = None,
                      dtype: Optional[torch.dtype] = None, attn_proj: Optional[tuple] = None):
        """(y, LN_consumer(y) in `dtype` | None) for small batches: the inner dimension split over `splits` workgroups per row
        block (ispk_ffn_bf16_prenorm2_split), then ONE pass that adds the partial products, the residual and the mask and
        already applies the norm that consumes the result (ispk_ffn_combine_ln_f32).  `attn_proj` = (attention output before
        to_out, Attention._chunked_wo()): x is the LAYER's input and the kernel applies to_out, mask and residual itself."""
        w1, _ = self._staged(torch.bfloat16)
        nn_ = None if consumer is None else (consumer.weight, consumer.bias, consumer.eps, consumer.apply_mask, dtype)
        return runtime.ffn_prenorm2_split(x, norm.weight, norm.bias, w1, self._chunked_w2(), mask, splits, next_norm=nn_,
                                          norm_eps=norm.eps, attn_proj=attn_proj)

    def lnin_gemm(self, x: Tensor, norm, mask: Optional[Tensor]) -> Tensor:
        """y = [mask] * (x + W2 act(W1 norm(x))) as two GEMMs, the LayerNorm applied by the first one while it stages x
        (ispk_gemm_bf16_lnin, statistics by its own waves); the `* mask` of transformer.py:102 is dead under the output mask."""
        w1, w2 = self._staged(torch.bfloat16)
        hidden = runtime.gemm_lnin(x, None, norm.weight, norm.bias, w1, bias=self.net[0].bias, flags=self.act_flag,
                                   ln_eps=norm.eps)
        return runtime.gemm(hidden, w2, bias=self.net[3].bias, resid=x, mask=mask,
                            flags=runtime.EP_MASK_OUT if mask is not None else 0, out_dtype=torch.float32)

    def forward(self, x: Tensor, *, residual: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                fused: Optional[bool] = None) -> Tensor:
        """`fused`: one kernel (ispk_ffn_bf16) instead of two GEMMs - a layer passes its plan's choice, a bare call (None)
        takes `plan.ffn_fused_ok` at the default seams."""
        if self.training and self.dropout_p > 0:
            raise NotImplementedError("feed-forward dropout (training) is outside the forward-path scope")
        dt = self.compute_dtype
        w1, w2 = self._staged(dt)
        flags = runtime.EP_MASK_OUT if mask is not None else 0
        if dt == torch.float16:   # split-fp16 path: x fp32 or split planes
            xs = x if x.dtype == torch.float16 else runtime.split_f16(x.float().contiguous())
            hidden = runtime.gemm_split(xs, w1, bias=self.net[0].bias, flags=self.act_flag, out_split=True)
            return runtime.gemm_split(hidden, w2, bias=self.net[3].bias, resid=residual, mask=mask, flags=flags)
        if x.dtype != dt:
            x = runtime.cast_bf16(x) if dt == torch.bfloat16 else x.float()
        if fused is None:
            fused = plan.ffn_fused_ok(dt, self.act_flag == runtime.EP_GELU, x.shape[-1], x.numel() // x.shape[-1], plan.SEAMS)
        if fused:   # the hidden activations never reach HBM
            return runtime.ffn_fused(x, w1, self._packed_w2(), resid=residual, mask=mask, bias1=self.net[0].bias,
                                     bias2=self.net[3].bias, flags=flags)
        hidden = runtime.gemm(x, w1, bias=self.net[0].bias, flags=self.act_flag)
        return runtime.gemm(hidden, w2, bias=self.net[3].bias, resid=residual, mask=mask, flags=flags,
                            out_dtype=torch.float32)
