"""Which kernels a `TransformerLayer` launches: ONE pure function of plain values (`select_plan`), the seams tests move
(`Seams`), and the typed hand-off between layers (`Consumer`, `Handed`).  Nothing here touches a tensor's contents or the
kernel library, so the table in DESIGN.md ("The layer plan") is pinned by a host test.
"""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum
from typing import Any, NamedTuple, Optional

import torch
from torch import Tensor

# ---- thresholds (rows = batch * positions) ----------------------------------------------------------------------------------
# The fused feed-forward kernels give a workgroup 128 rows and the whole inner dimension: with 128 row blocks or fewer
# (<= 16,384 rows: half the chip) the split form - several workgroups per row block, each a slice of the inner dimension, + one
# combine pass - fills the CUs instead (dim 384); other dims take the two-GEMM path there.  Also the floor of the two-GEMM
# path's LayerNorm-inside-the-first-GEMM: below, the separate LayerNorm launch is cheaper (28.8 vs 19.4 + 4.9 us at 6,400 rows:
# every workgroup of the split output repeats the fp32 staging).
FUSED_MIN_ROWS = 128 * 128 + 1
# LayerNorm inside the q/kv GEMM with statistics computed by the GEMM's own waves: pays from decoder-sized batches on (33.0 vs
# 22.1 + 15.0 us at 32,768 rows); at 6,400 rows the output is split over many workgroups that each repeat the fp32 staging, and
# the separate 4.9-us LayerNorm is cheaper (18.6 vs 9.4 + 4.9 us).  One row less than FUSED_MIN_ROWS on purpose: 16,384 rows
# take this q/kv GEMM and the 2-way split feed-forward.
LNIN_SELF_MIN_ROWS = 128 * 128
# Split feed-forward (text encoder: 6,400 rows = 50 row blocks on 256 CUs; 22.4 (FFN2) + 19.8 (FFN1) + 7.1 (LayerNorm) + 5.8
# (next LayerNorm) us as separate launches -> measured in DESIGN.md): from one row block on (at 8 utterances per GPU the text
# encoder has 800 rows) ...
SPLIT_MIN_ROWS = 128
# ... over at most 8 workgroups per row block (16 measured no faster at 800 rows: the combine pass reads every partial)
MAX_SPLITS = 8
# to_out in every workgroup of the split feed-forward pays with 2 splits (16,384 decoder rows = 32 utterances per GPU: 1.512 ->
# 1.498 ms per step); with 4 - 8 splits per row block the repeated projection costs more than the to_out launch it saves (6,400
# rows: 2.004 -> 2.012 ms; 8 utterances per GPU: 1.014 -> 1.066 ms)
PROJ_FFN_SPLIT_MIN_ROWS = 8192

# The short-sequence attention block as ONE kernel (ispk_attn_block_short_bf16: q/kv projection, attention, to_out with mask and
# residual) instead of three launches: at most 128 positions per batch item (the whole key range of an item sits in one
# workgroup's LDS), dims 256 / 384 with 64-wide heads.
SHORT_BLOCK_MAX_N = 128
# ... and from this many rows on, per dim.  The kernel itself beats the three launches at every size (tools/bench_attn_block.py,
# per block, 64 / 8 / 1 utterances of 100 positions: dim 384 30.5 -> 21.8, 20.0 -> 19.4, 19.4 -> 19.3 us; dim 256 22.0 -> 14.7,
# 16.3 -> 12.9, 15.8 -> 12.9 us); the threshold is set by the graphed step (tools/ab_switches.py, switch off minus on, and the
# spread of two captures of one configuration):
#   dim 384, the text encoder's six layers:  +36 us at 6,400 rows (spread 2), +12 .. 20 at 3,200 (9), +9 .. 17 at 1,600 (8),
#                                            +23 at 800 (0.3): on from one 128-row block (`SPLIT_MIN_ROWS`) - below it a
#                                            stack is the plain seven launches that the hand-off tests count, and one
#                                            utterance of 100 rows gains nothing anyway (19.4 -> 19.3 us a block);
#   dim 256, the flow predictor's three layers, which run on the side stream beside the decoder: +27 us at 6,400 rows (spread 2),
#                                            -3 .. -12 at 3,200 (9), -1 .. +8 at 1,600 (8), -5.5 at 800 (0.3) - its 512-thread workgroups
#                                            with 114 KB of LDS take CUs from the decoder's kernels there: on from the one
#                                            size at which it is measured to win.
# (The embedding stack's single dim-256 layer gains 2.5 us at 6,400 rows and 3.1 at 800 - not clear of three times the spread:
# `TransformerTemporalModule` leaves its switch off.)
SHORT_BLOCK_MIN_ROWS = {384: 128, 256: 6400}


@dataclass(frozen=True)
class Seams:
    """The switches tests move to reach the unfused path they compare against.  `SEAMS` is the default; a `Transformer` (or one
    `TransformerLayer` call) takes its own through `seams`.  Nothing reads the environment."""
    prenorm_fused: bool = True     # norm -> feed-forward -> residual as one kernel (ispk_ffn_bf16_prenorm / _prenorm2) and what builds on it
    lnin_self: bool = True         # LayerNorm applied by the consuming GEMM's own waves (ispk_gemm_bf16_lnin, row_stats = NULL)
    next_qkv: bool = True          # ispk_attn_out_ffn_qkv_bf16: the next layer's attention_norm + q/kv projection as the kernel's epilogue
    proj_ffn: bool = True          # to_out + residual + norm + feed-forward + residual as ONE kernel (ispk_attn_out_ffn_bf16)
    proj_ffn_split: bool = True    # ... and in every workgroup of the split feed-forward (ispk_attn_out_ffn_split_bf16)
    # The LayerNorm that consumes a layer's output moves only its STATISTICS: the fused feed-forward kernel writes (mean, rstd)
    # per row and the next layer's q/kv GEMM normalises while it stages its fp32 input - no normalised copy in HBM (q/kv 21.8 ->
    # 26.6 us, the 15.0-us LayerNorm launch disappears: 2.636 -> 2.587 ms per step).  Off: no layer is asked to hand anything on.
    stats_layernorm: bool = True
    fused_min_rows: int = FUSED_MIN_ROWS
    lnin_self_min_rows: int = LNIN_SELF_MIN_ROWS


SEAMS = Seams()


class Qkv(Enum):    # where a layer's q/kv rows come from
    HANDED_QKV = "q/kv rows from the previous layer's kernel"
    LNIN_STATS = "gemm_lnin with the previous layer's row statistics"
    LNIN_SELF = "gemm_lnin with its own statistics"
    HANDED_ROWS = "GEMM on the normalised rows the previous layer's combine pass wrote"
    NORM_GEMM = "attention_norm launch + GEMM"


class Form(Enum):    # the second half of a layer: everything after the attention kernel
    ATTN_OUT_FFN = "attn_out_ffn"
    ATTN_OUT_FFN_STATS = "attn_out_ffn + row statistics"
    ATTN_OUT_FFN_QKV = "attn_out_ffn + the next layer's q/kv"
    ATTN_OUT_FFN_NORM = "attn_out_ffn + the stack's final norm"
    FFN_PRENORM2 = "to_out, ffn_prenorm2 (eight waves)"
    FFN_PRENORM = "to_out, ffn_prenorm (four waves)"
    SPLIT = "to_out, split feed-forward + combine"
    SPLIT_PROJ = "split feed-forward with the to_out prologue + combine"
    LNIN_GEMM = "to_out, gemm_lnin, GEMM"
    NORM_FFN_FUSED = "to_out, norm, ffn_fused"
    NORM_FFN_GEMMS = "to_out, norm, two GEMMs"
    SPLIT_FP16 = "the seven launches on the split-fp16 kernels"


ATTN_OUT_FFN_FORMS = (Form.ATTN_OUT_FFN, Form.ATTN_OUT_FFN_STATS, Form.ATTN_OUT_FFN_QKV, Form.ATTN_OUT_FFN_NORM)


class Hand(Enum):    # what passes from one layer to the consumer of its output beside `out`
    NONE = "nothing"
    STATS = "row statistics (mean, rstd) of the consuming LayerNorm"
    QKV = "the next layer's q/kv rows"
    ROWS = "the consuming LayerNorm's output rows"


class Next(Enum):    # what consumes a layer's output
    NONE = "the caller, raw"
    LAYER = "the next layer's attention_norm"
    FINAL = "the stack's final norm"


class Plan(NamedTuple):
    qkv: Qkv
    defer_out: bool                  # to_out is applied by the second half's kernel; the attention block returns its input
    form: Form
    splits: int = 0                  # SPLIT / SPLIT_PROJ: workgroups per row block
    hands: Hand = Hand.NONE
    hand_dtype: Optional[torch.dtype] = None    # Hand.ROWS: their dtype
    store_out: bool = True           # False: only what is handed on is written (`out` is None)


class Consumer(NamedTuple):
    """The LayerNorm that consumes a layer's output, as the kernels that can apply it need it."""
    kind: Next = Next.NONE
    weight: Optional[Tensor] = None
    bias: Optional[Tensor] = None
    eps: float = 1e-5
    apply_mask: bool = False                     # Next.FINAL: the stack's final norm is row-masked
    dtype: Optional[torch.dtype] = None          # Next.FINAL: the dtype its rows are wanted in
    attention: Any = None                        # Next.LAYER: the next layer's Attention (heads, dim, q/kv weights)
    only_normed: bool = False                    # Next.FINAL: the caller reads nothing but the norm's rows


class Handed(NamedTuple):
    """What a layer's kernels produced for the consumer of its output."""
    kind: Hand = Hand.NONE
    tensor: Optional[Tensor] = None


def ffn_fused_ok(cdt: torch.dtype, gelu: bool, dim: int, rows: int, seams: Seams) -> bool:
    """`FeedForward.forward` on normalised rows: the four-wave kernel for Linear -> GELU -> Linear (ispk_ffn_bf16, the hidden
    activations never reach HBM) instead of two GEMMs."""
    return cdt == torch.bfloat16 and gelu and dim in (256, 384) and rows >= seams.fused_min_rows


def split_count(rows: int, inner: int) -> int:
    """Workgroups per 128-row block of the split feed-forward: as many as fit one round of the 256 CUs, at least 2 chunks of 32
    inner columns each."""
    chunks, blocks, splits = inner // 32, (rows + 127) // 128, 1
    for s in (2, 3, 4, 6, 8):
        if s <= MAX_SPLITS and chunks % s == 0 and chunks // s >= 2 and blocks * s <= 256:
            splits = s
    return splits


def select_plan(*, cdt: torch.dtype, dim: int, heads: int, out_dim: int, inner: int, rows: int, plain_norms: bool,
                bias1: bool, bias2: bool, gelu: bool, dropout: bool, prev: Hand = Hand.NONE, consumer: Next = Next.NONE,
                consumer_dtype: Optional[torch.dtype] = None, next_heads: int = 0, next_dim: int = 0,
                only_normed: bool = False, seams: Optional[Seams] = None) -> Plan:
    """The kernels one pre-norm layer launches.
    `cdt`: fp32, bf16 or fp16 (= split fp16).  `plain_norms`: both norms are LayerNorms with weight and bias (else adaptive or
    non-affine).  `bias1` / `bias2`: the feed-forward's Linears have one; `dropout`: training with feed-forward dropout.
    `prev`: what the previous layer handed over.  `consumer` (+ `consumer_dtype` for the final norm, `next_heads` / `next_dim`
    for a layer): what reads this layer's output; `only_normed`: and reads nothing but the final norm's rows.  `seams`: None =
    the module's `SEAMS` as it is at the call."""
    seams = seams or SEAMS
    if cdt == torch.float16:
        return Plan(Qkv.NORM_GEMM, False, Form.SPLIT_FP16)
    bf = cdt == torch.bfloat16
    # what this layer is asked to hand on: bf16, plain LayerNorms only
    if not (seams.stats_layernorm and plain_norms and bf) or (
            consumer is Next.FINAL and consumer_dtype not in (torch.float32, torch.bfloat16)):
        consumer = Next.NONE
    ff = plain_norms and bf and not dropout          # the feed-forward kernels that apply feed_forward_norm themselves
    prenorm = seams.prenorm_fused and ff and gelu and dim in (256, 384) and rows >= seams.fused_min_rows and not bias1
    pair = dim == 384 and not bias2 and inner % 32 == 0          # the eight-wave kernel (csrc/ffn2.hip), else the four-wave one
    proj = bf and seams.proj_ffn and out_dim == dim and prenorm and pair and inner >= 64
    split = (ff and gelu and dim == 384 and SPLIT_MIN_ROWS <= rows < seams.fused_min_rows and not bias1 and not bias2
             and inner % 64 == 0)
    proj_split = (not proj and split and seams.proj_ffn_split and out_dim == dim == 384 and rows >= PROJ_FFN_SPLIT_MIN_ROWS)

    if prev is Hand.QKV:
        qkv = Qkv.HANDED_QKV
    elif prev is Hand.STATS:
        qkv = Qkv.LNIN_STATS
    elif prev is Hand.ROWS:
        qkv = Qkv.HANDED_ROWS
    elif bf and plain_norms and dim in (256, 384) and seams.lnin_self and rows >= seams.lnin_self_min_rows:
        qkv = Qkv.LNIN_SELF
    else:
        qkv = Qkv.NORM_GEMM
    assert bf or prev is Hand.NONE

    if proj:
        if consumer is Next.FINAL:
            return Plan(qkv, True, Form.ATTN_OUT_FFN_NORM, 0, Hand.ROWS, consumer_dtype, not only_normed)
        if consumer is Next.LAYER and seams.next_qkv and next_heads * 64 + 128 == 512 and next_dim == dim:
            return Plan(qkv, True, Form.ATTN_OUT_FFN_QKV, 0, Hand.QKV)
        if consumer is Next.LAYER:
            return Plan(qkv, True, Form.ATTN_OUT_FFN_STATS, 0, Hand.STATS)
        return Plan(qkv, True, Form.ATTN_OUT_FFN)
    if prenorm:       # (the stack's final norm is not served here: a launch of its own)
        return Plan(qkv, False, Form.FFN_PRENORM2 if pair else Form.FFN_PRENORM, 0,
                    Hand.STATS if consumer is Next.LAYER else Hand.NONE)
    if split:
        # the combine pass already applies the norm that consumes the result: the next layer's in the compute dtype, the
        # stack's final one in the dtype its caller asked for
        hands, hdt = Hand.NONE, None
        if consumer is not Next.NONE:
            hands, hdt = Hand.ROWS, torch.float32 if (consumer is Next.FINAL and consumer_dtype == torch.float32) else cdt
        return Plan(qkv, proj_split, Form.SPLIT_PROJ if proj_split else Form.SPLIT, split_count(rows, inner), hands, hdt)
    if seams.lnin_self and ff and dim in (256, 384) and rows >= seams.fused_min_rows:
        # two-GEMM feed-forward (e.g. an activation the fused kernel lacks): feed_forward_norm inside the first Linear's GEMM
        return Plan(qkv, False, Form.LNIN_GEMM)
    return Plan(qkv, False, Form.NORM_FFN_FUSED if ffn_fused_ok(cdt, gelu, dim, rows, seams) else Form.NORM_FFN_GEMMS)


def short_block_ok(*, cdt: torch.dtype, tape: bool, residual: bool, defer_out: bool, n: int, heads: int, dim: int, out_dim: int,
                   rows: int) -> bool:
    """`Attention.forward` (consulted when its `short_block` switch is on): may this call be ONE ispk_attn_block_short_bf16
    launch?  bf16 forward without a tape, the residual fused into to_out (so not `defer_out`, where the next kernel applies
    to_out), at most SHORT_BLOCK_MAX_N positions, heads * 64 = dim in {256, 384}, and enough rows for the kernel to win.
    Independent of `select_plan`: the plan decides which tensors reach the attention block, this only how it launches."""
    return (cdt == torch.bfloat16 and not tape and residual and not defer_out and 1 <= n <= SHORT_BLOCK_MAX_N
            and dim in SHORT_BLOCK_MIN_ROWS and heads * 64 == dim == out_dim and rows >= SHORT_BLOCK_MIN_ROWS[dim])
