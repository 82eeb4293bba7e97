"""`TransformerLayer` / `Transformer` (tts/modules/transformer/transformer.py:37-211 of the reference).

Pre-norm layer with nothing fused (7 kernels, activations make one HBM round trip between them): the exact-fp32 path, the
split-fp16 path (the same seven on csrc/split.hip's kernels, operands as hi / lo fp16 planes), adaptive norms, bf16 below 128 rows
    h  = LN/AdaLN(x)                                   ispk_layernorm
    qkv = h · [Wq;Wkv]ᵀ                                ispk_gemm
    o  = ALiBi-MQA(qkv)                                ispk_alibi_mqa_attn
    x1 = x + mask * (o · Woᵀ)                          ispk_gemm, epilogue MASK_ACC + residual   (transformer.py:91)
    h2 = mask * LN/AdaLN(x1)                           ispk_layernorm with row mask             (:97-102)
    f  = gelu(h2 · W1ᵀ)                                ispk_gemm, epilogue GELU
    y  = mask * (x1 + f · W2ᵀ)                         ispk_gemm, epilogue residual + MASK_OUT   (:105-110)
The residual stream (x, x1, y) is always fp32; with compute_dtype = bf16 the GEMM/attention operands are bf16.

bf16 path, plain LayerNorms: `plan.select_plan` folds these launches into each other by the stack's size (table: DESIGN.md 4.1d).
Dim 384 from 16,385 rows (decoder): TWO launches a layer, attention and ispk_attn_out_ffn_qkv_bf16 (to_out, y and the NEXT layer's
q/kv rows; the last layer's writes the stack's final norm instead).  Dim 384, 128 .. 16,384 rows (text encoder): the feed-forward
split over the inner dimension + one combine pass that applies the consuming LayerNorm, 5 launches a layer (4 from 8,192 rows).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import NamedTuple, Optional, Union

import torch
import torch.nn as nn
from torch import Tensor

from ... import runtime
from ...staging import StagedWeights
from ..constructor import Constructor, ModuleConfig
from .attend import AttentionIntermediates
from .attention import Attention, AttentionConfig, AttentionSharedIntermediates
from .feedforward import FeedForward, FeedForwardConfig
from .normalization import AdaptiveLayerNorm, LayerNorm
from .plan import ATTN_OUT_FFN_FORMS, Consumer, Form, Hand, Handed, Next, Plan, Qkv, Seams, select_plan


class TransformerLayerIntermediates(NamedTuple):
    attention: Optional[AttentionIntermediates] = None


class TransformerLayerOutput(NamedTuple):
    out: Optional[Tensor]            # (None when the plan stores only what it hands on)
    intermediates: Optional[TransformerLayerIntermediates] = None
    shared_intermediates: Optional[AttentionSharedIntermediates] = None
    handed: Handed = Handed()        # what the layer's kernels already produced for the consumer of `out` (not in the reference)


@dataclass
class TransformerLayerConfig(ModuleConfig):
    dim: int = 384
    attention: Union[AttentionConfig, dict] = field(default_factory=AttentionConfig)
    feed_forward: Union[FeedForwardConfig, dict] = field(default_factory=FeedForwardConfig)
    pre_norm: bool = True
    adaptive_norm: bool = False
    condition_dim: Optional[int] = None


class TransformerLayer(nn.Module, Constructor):
    def __init__(self, dim: int = 384, attention=None, feed_forward=None, pre_norm: bool = True,
                 adaptive_norm: bool = False, condition_dim: Optional[int] = None):
        super().__init__()
        if not pre_norm:
            raise NotImplementedError("post-norm layers are unused by the recipes and not built")
        assert not adaptive_norm or condition_dim is not None
        self.pre_norm, self.adaptive_norm = pre_norm, adaptive_norm
        norm = (lambda: AdaptiveLayerNorm(dim, condition_dim=condition_dim)) if adaptive_norm else (lambda: LayerNorm(dim))
        self.attention_norm = norm()
        self.attention = Attention.init(attention if attention is not None else AttentionConfig(), dim=dim)
        self.feed_forward_norm = norm()
        self.feed_forward = FeedForward.init(feed_forward if feed_forward is not None else FeedForwardConfig(), dim=dim)

    def _plan(self, dim: int, rows: int, prev: Handed, consumer: Consumer, seams: Optional[Seams]) -> Plan:
        """This layer's facts as plain values, through `select_plan`."""
        att, ff = self.attention, self.feed_forward
        plain = all(isinstance(n, nn.LayerNorm) and n.weight is not None and n.bias is not None
                    for n in (self.attention_norm, self.feed_forward_norm))
        nxt = consumer.attention
        return select_plan(cdt=att.compute_dtype, dim=dim, heads=att.heads, out_dim=att.out_dim, inner=ff.net[0].weight.shape[0],
                           rows=rows, plain_norms=plain, bias1=ff.net[0].bias is not None, bias2=ff.net[3].bias is not None,
                           gelu=ff.act_flag == runtime.EP_GELU, dropout=ff.training and ff.dropout_p > 0, prev=prev.kind,
                           consumer=consumer.kind, consumer_dtype=consumer.dtype, next_heads=nxt.heads if nxt is not None else 0,
                           next_dim=nxt.dim if nxt is not None else 0, only_normed=consumer.only_normed, seams=seams)

    def forward(self, x: Tensor, mask: Optional[Tensor] = None, context: Optional[Tensor] = None,
                context_mask: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None,
                adaptive_condition: Optional[Tensor] = None, cache: Optional[TransformerLayerIntermediates] = None,
                shared_cache: Optional[AttentionSharedIntermediates] = None, *, key_len: Optional[Tensor] = None,
                ada: Optional[tuple] = None, prev: Handed = Handed(), consumer: Consumer = Consumer(),
                seams: Optional[Seams] = None):
        """`ada`: the (scale, shift) pairs of the two adaptive norms, already projected from the condition.  `prev`: what the
        previous layer's kernels already produced of this layer's attention_norm.  `consumer`: the LayerNorm that will read this
        layer's output - where the plan's kernels can serve it, the output carries the result in `handed` (and `out` is None if
        the consumer reads nothing else).  `seams`: the path switches, None = `plan.SEAMS`."""
        assert not self.adaptive_norm or adaptive_condition is not None or ada is not None, \
            "`adaptive_condition` should be provided for AdaptiveLayerNorm"
        if cache is not None:
            raise NotImplementedError("KV caches are not on the acoustic-model forward path")
        if context is not None or context_mask is not None or attention_mask is not None:
            raise NotImplementedError("cross-attention / explicit attention masks are not on the forward path")
        x = x.float().contiguous()
        if mask is not None and key_len is None:
            key_len = mask.sum(dim=1)
        att, ff, fn = self.attention, self.feed_forward, self.feed_forward_norm
        cdt = att.compute_dtype
        p = self._plan(x.shape[-1], x.numel() // x.shape[-1], prev, consumer, seams)

        def norm(n, t: Tensor, scale_shift: Optional[tuple], row_mask: Optional[Tensor] = None) -> Tensor:
            if cdt == torch.float16:   # (split fp16 planes out)
                return self._norm_split(n, t, adaptive_condition, scale_shift, row_mask)
            kw = {} if scale_shift is None else {"scale_shift": scale_shift}
            return n(t, adaptive_condition, row_mask=row_mask, out_dtype=cdt, **kw)

        qkv = None
        if p.qkv is Qkv.HANDED_QKV:
            qkv = prev.tensor
        elif p.qkv in (Qkv.LNIN_STATS, Qkv.LNIN_SELF):
            qkv = att.qkv_lnin(x, self.attention_norm, prev.tensor if p.qkv is Qkv.LNIN_STATS else None)
        h = x if qkv is not None else prev.tensor if p.qkv is Qkv.HANDED_ROWS else norm(self.attention_norm, x, ada and ada[0])
        # (with `defer_out`, x1 is the attention output before to_out)
        x1, inter, shared = att(h, mask=mask, key_len=key_len, residual=x, qkv=qkv, defer_out=p.defer_out)

        second = None
        served = consumer if p.hands is not Hand.NONE else None
        if p.form in ATTN_OUT_FFN_FORMS:
            y, second = ff.attn_out_ffn(x, x1, att._chunked_wo(), fn, mask, p.form, served, p.store_out)
        elif p.form in (Form.FFN_PRENORM2, Form.FFN_PRENORM):
            y, second = ff.prenorm(x1, fn, mask, p.form is Form.FFN_PRENORM2, served.eps if served is not None else None)
        elif p.form is Form.SPLIT_PROJ:
            y, second = ff.prenorm_split(x, fn, mask, p.splits, served, p.hand_dtype, attn_proj=(x1, att._chunked_wo()))
        elif p.form is Form.SPLIT:
            y, second = ff.prenorm_split(x1, fn, mask, p.splits, served, p.hand_dtype)
        elif p.form is Form.LNIN_GEMM:
            y = ff.lnin_gemm(x1, fn, mask)
        else:   # NORM_FFN_FUSED, NORM_FFN_GEMMS, SPLIT_FP16
            y = ff(norm(fn, x1, ada and ada[1], mask), residual=x1, mask=mask, fused=p.form is Form.NORM_FFN_FUSED)
        return TransformerLayerOutput(out=y, intermediates=TransformerLayerIntermediates(attention=inter),
                                      shared_intermediates=shared, handed=Handed(p.hands, second))

    def _norm_split(self, norm, x: Tensor, condition: Optional[Tensor], scale_shift: Optional[tuple],
                    row_mask: Optional[Tensor]) -> Tensor:
        """LayerNorm / AdaptiveLayerNorm with the result as split fp16 planes (ispk_layernorm_f32_split)."""
        if isinstance(norm, AdaptiveLayerNorm):
            if scale_shift is None and condition is not None:
                cond = condition.reshape(-1, condition.shape[-1]).float().contiguous()
                scale_shift = (runtime.linear_small(cond, norm.weight.weight, norm.weight.bias),
                               runtime.linear_small(cond, norm.bias.weight, norm.bias.bias) if norm.bias is not None else None)
            if scale_shift is None:
                return runtime.layernorm_split(x, None, None, row_mask=row_mask, eps=norm.eps)
            rows_per_batch = x.numel() // (x.shape[0] * x.shape[-1])
            return runtime.layernorm_split(x, None, None, scale_shift[0], scale_shift[1], rows_per_batch, row_mask, norm.eps)
        return runtime.layernorm_split(x, norm.weight, norm.bias, row_mask=row_mask, eps=norm.eps)


class TransformerOutput(NamedTuple):
    out: Tensor
    intermediates: Optional[list] = None


@dataclass
class TransformerConfig(ModuleConfig):
    dim: int = 384
    depth: int = 6
    transformer_layer: Union[TransformerLayerConfig, dict] = field(default_factory=TransformerLayerConfig)
    emb_dim: Optional[int] = None
    use_abs_pos_emb: bool = True
    adaptive_norm: bool = False
    condition_dim: Optional[int] = None


class Transformer(nn.Module, Constructor):
    seams: Optional[Seams] = None    # this stack's path switches (set on an instance; tests): None = `plan.SEAMS`

    def __init__(self, dim: int = 384, depth: int = 6, transformer_layer=None, emb_dim: Optional[int] = None,
                 use_abs_pos_emb: bool = True, adaptive_norm: bool = False, condition_dim: Optional[int] = None):
        super().__init__()
        self.dim = dim
        self.emb_dim = emb_dim = emb_dim or dim
        self.adaptive_norm = adaptive_norm
        layer_cfg = transformer_layer if transformer_layer is not None else TransformerLayerConfig()
        self.layers = nn.ModuleList([
            TransformerLayer.init(layer_cfg, dim=dim, adaptive_norm=adaptive_norm, condition_dim=condition_dim)
            for _ in range(depth)])
        if use_abs_pos_emb and self.layers[0].attention.rel_pos is None:
            raise NotImplementedError("absolute sinusoidal position embeddings (no ALiBi) are unused by the recipes")
        self.pos_emb = None
        self.project_emb = nn.Linear(emb_dim, dim) if emb_dim != dim else nn.Identity()  # transformer.py:170
        self.norm = nn.LayerNorm(dim)                                                      # transformer.py:172
        self._ada_cache = StagedWeights()

    def _ada_all(self, condition: Tensor):
        """Projects the condition for every AdaptiveLayerNorm of the stack in ONE launch (2 norms x 2 Linears per layer
        would otherwise be 4*depth tiny launches): concatenated [4*depth*dim, cond] weight, sliced per norm."""
        norms = [n for layer in self.layers for n in (layer.attention_norm, layer.feed_forward_norm)]
        ps = [p for n in norms for p in (n.weight.weight, n.weight.bias, n.bias.weight, n.bias.bias)]

        def build():
            with torch.no_grad():
                return (torch.cat([torch.cat([n.weight.weight, n.bias.weight]) for n in norms]).contiguous(),
                        torch.cat([torch.cat([n.weight.bias, n.bias.bias]) for n in norms]).contiguous())
        w_all, b_all = self._ada_cache.get("ada", ps, build)
        cond = condition.reshape(-1, condition.shape[-1]).float().contiguous()
        proj = runtime.linear_small(cond, w_all, b_all)       # [Bc, 2*len(norms)*dim]
        d = self.dim
        parts = [(proj[:, (2 * i) * d:(2 * i + 1) * d], proj[:, (2 * i + 1) * d:(2 * i + 2) * d])
                 for i in range(len(norms))]
        return [(parts[2 * li], parts[2 * li + 1]) for li in range(len(self.layers))]

    def set_compute_dtype(self, dtype: torch.dtype):
        """fp32 (exact-fp32 MFMAs), bf16 (throughput path) or fp16 = the split-fp16 path: fp32-grade products as three fp16
        MFMAs over hi / lo terms (csrc/split.hip)."""
        assert dtype in (torch.float32, torch.bfloat16, torch.float16)
        for layer in self.layers:
            layer.attention.compute_dtype = dtype
            layer.feed_forward.compute_dtype = dtype
        return self

    def _consumer(self, li: int, mask: Optional[Tensor], out_dtype: torch.dtype, final_norm: bool) -> Consumer:
        """The LayerNorm that reads layer `li`'s output: the next layer's attention_norm or, after the last layer, the stack's
        own final norm (row-masked, transformer.py:205-206), which is all the caller then reads.  Whether a layer's kernels
        serve it is the plan's decision."""
        if li + 1 < len(self.layers):
            nxt = self.layers[li + 1]
            c = Consumer(Next.LAYER, nxt.attention_norm.weight, nxt.attention_norm.bias, nxt.attention_norm.eps,
                         attention=nxt.attention)
        else:
            c = Consumer(Next.FINAL, self.norm.weight, self.norm.bias, self.norm.eps, mask is not None, out_dtype,
                         only_normed=True)
        served = not self.adaptive_norm and (li + 1 < len(self.layers) or final_norm)
        return c if served and c.weight is not None and c.bias is not None else Consumer()

    def forward(self, x: Tensor, mask: Optional[Tensor] = None, context: Optional[Tensor] = None,
                context_mask: Optional[Tensor] = None, attention_mask: Optional[Tensor] = None,
                adaptive_condition: Optional[Tensor] = None, return_intermediates: bool = False, *,
                key_len: Optional[Tensor] = None, projected: Optional[Tensor] = None,
                out_dtype: torch.dtype = torch.float32, final_norm: bool = True, handed: Handed = Handed()):
        """`handed`: what the caller's kernels already produced of layer 0's attention_norm over `x` (`Handed(Hand.QKV, rows)`: its
        q/kv rows) - layer 0 then plans as any layer does behind a producing one.
        `final_norm=False`: `.out` is the last layer's raw output - for a caller whose next kernel applies `self.norm` itself
        (the flow predictor's head, `runtime.flow_head`).
        `projected` lets a caller that already holds project_emb(x) (e.g. the Euler loop, which re-projects only the
        3 flow channels per step) skip the projection.  `out_dtype=torch.bfloat16` makes the final LayerNorm emit bf16
        for a bf16 consumer (the decoder's to_mel GEMM on the bf16 path)."""
        if projected is not None:
            out = projected
        elif isinstance(self.project_emb, nn.Identity):
            out = x.float()
        else:
            out = runtime.linear(x.float(), self.project_emb.weight, self.project_emb.bias)   # (strided rows are fine)
        if mask is not None and key_len is None:
            key_len = mask.sum(dim=1)
        intermediates = []
        ada = self._ada_all(adaptive_condition) if (self.adaptive_norm and adaptive_condition is not None) else None
        for li, layer in enumerate(self.layers):
            res = layer(out, mask=mask, context=context, context_mask=context_mask, attention_mask=attention_mask,
                        adaptive_condition=adaptive_condition, key_len=key_len, ada=None if ada is None else ada[li],
                        prev=handed, consumer=self._consumer(li, mask, out_dtype, final_norm), seams=self.seams)
            out, handed = res.out, res.handed
            if return_intermediates:
                intermediates.append(res.intermediates)
        if not final_norm:
            return TransformerOutput(out=out, intermediates=intermediates)
        if handed.kind is Hand.ROWS:     # the last layer's kernel already applied the final norm
            normed = handed.tensor
        elif out_dtype == torch.float16:   # split fp16 planes [2, B, N, D] for a split-fp16 consumer GEMM
            normed = runtime.layernorm_split(out, self.norm.weight, self.norm.bias, row_mask=mask, eps=self.norm.eps)
        else:
            normed = runtime.layernorm(out, self.norm.weight, self.norm.bias, row_mask=mask, eps=self.norm.eps,
                                       out_dtype=out_dtype)
        return TransformerOutput(out=normed, intermediates=intermediates)
