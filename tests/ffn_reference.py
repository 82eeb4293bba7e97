"""Float64 references of the fused feed-forward kernels (csrc/ffn.hip, csrc/ffn2.hip), written from the statements in
include/ispk.h (no call into isp_tts_amd), plus the case tables, the seeded inputs, the bound and the deliberately wrong
references ("mutants") that tests/test_ffn_reference_host.py and tests/test_gpu_ffn_kernels.py share.

Two evaluations per reference
  exact     float64 throughout.
  rounded   float64 with the kernels' stated roundings and nothing else: LN(x) to bf16 before the first product, the hidden
            activations to bf16 before the second, LN_next(out) to bf16 before the q/kv product, bf16 outputs where the entry
            stores bf16.  (ispk_ffn_bf16 takes bf16 rows: its only rounding is the hidden one.)

The bound (`ratios`)
  e_round = |rounded - exact| per case and output, as max and as rms; for a case of fewer than 128 rows it is taken from the
  same inputs extended to 128 rows (`bound_rows`), so that a lucky small sample cannot shrink it.  A kernel passes when
      max |kernel - exact| <= FACTOR     x max e_round      FACTOR = 3.0: the project's figure for "same roundings, another
      rms |kernel - exact| <= RMS_FACTOR x rms e_round      order" (BF16_FACTOR of the vocoder tests); RMS_FACTOR = 1.5:
  independent errors add in quadrature, the eight-wave GELU's stated error (an eighth of a bf16 step against rounding's
  1 / sqrt 12 of a step rms) adds under 10 %, fp32 summation order far less; 1.5 is margin over that.  e_round itself stays
  under what tests/test_gpu_kernels.py allows (CEIL_MAX / CEIL_RMS, CEIL_QKV), asserted on the CPU by the host test, so the
  bound is never looser than the old one.  Where every kept value of a case is exactly representable (all rows masked)
  e_round is 0 and the kernel has to be exact.  (The 128-row extension of a short case follows the case's mask pattern: under
  `prefix` 50 of its rows are masked and add no error, so the rms allowance of a case whose own rows are all valid is tighter
  by sqrt(78 / 128) - stricter, never looser; the kernels pass it, see the table in tests/test_gpu_ffn_kernels.py.)
  The derived outputs are checked against float64 of the kernel's OWN rows with the figures of tests/test_gpu_kernels.py:
  statistics (mean 1e-6, rstd 1e-5 relative), LayerNorm outputs (2e-5 fp32, 2^-7 bf16, x max(1, max |ref|)), q/kv by the
  FACTOR rule against LN_next of the kernel's rows.  `ratios` returns every figure divided by its allowance: <= 1 passes.

Inputs: seeded normals as in tests/test_gpu_kernels.py (x mean 1.5 std 0.4, W1 ~ dim^-1/2, W2 ~ inner^-1/2, weights rounded to
bf16), NROWS rows per (dim, inner) of which a case takes the first R - so R + k rows are the same rows with k appended.  One
addition: row CONST_ROW of x is the constant 1.5 and its attention-output row is 0, a row without variance, so that a
LayerNorm without eps shows (0 x inf) instead of hiding 3e-5 below the bf16 rounding of the normalised row.

Flag placement, as the header states it (and as the kernels do it):
  ispk_ffn_bf16[_prenorm[2]]   v = ffn (+ bias2); MASK_ACC: v *= mask; v += resid | x; MASK_OUT: v *= mask
  ispk_attn_out_ffn_*          MASK_ACC masks the projection (x1 = x + mask * o Wo^T), MASK_OUT the output rows
  ispk_attn_out_ffn_split      MASK_ACC only; the combine pass masks y

Mutants: one-line changes of `rounded` (MUTANTS).  "Hidden units of a chunk in pack_w2 order instead of natural order" and
its reverse are ONE mutant: the packing permutation swaps bits 2 and 3 of the position, it is its own inverse.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

F64 = torch.float64
BF16 = torch.bfloat16
GELU, MASK_ACC, MASK_OUT = 1, 4, 8
FACTOR, RMS_FACTOR = 3.0, 1.5
CEIL_MAX, CEIL_RMS, CEIL_QKV = 0.06, 6e-3, 0.08        # tests/test_gpu_kernels.py, against float64
STATS_MEAN_TOL, STATS_RSTD_TOL = 1e-6, 1e-5
LN_TOL = {False: 2e-5, True: 2.0 ** -7}                 # fp32 / bf16 LayerNorm output, x max(1, max |ref|)
EPS = float(np.float32(1e-5))                           # every eps of the tests, as the C entry points receive it
NROWS = 400                                             # rows of an input set: 257 + 130 appended fit
CONST_ROW = 100
NQ = 512


# ------------------------------------------------------------------------------------------------ case tables

ROWS = (1, 16, 17, 32, 33, 64, 65, 127, 128, 129, 257)
INNER2 = (32, 64, 96, 128, 160)
ROWS4 = (1, 31, 32, 33, 127, 128, 129)
INNER4 = (64, 96, 160)
SPLIT_CASES = ((129, 64, 1), (129, 128, 2), (17, 192, 3), (129, 192, 2), (257, 1536, 24), (130, 1536, 16), (1, 128, 2))
MASKS = ("none", "ones", "prefix", "tile", "zeros")
FLAG_SETS = (0, MASK_OUT, MASK_ACC, MASK_ACC | MASK_OUT)
COMBINE_ROWS, COMBINE_SPLITS = (1, 7, 8, 9, 257), (1, 2, 3, 16)


def shapes2(min_inner=32):
    """(R, inner, mask of the shape's main case) of an eight-wave entry: every R at inner 96, every inner at R = 129, (257, 160)
    with the all-masked tile, one production-size inner."""
    s = [(r, 96, "prefix") for r in ROWS] + [(129, i, "prefix") for i in INNER2 if i >= min_inner and i != 96]
    return s + [(257, 160, "tile"), (129, 1536, "prefix")]


def shapes4():
    return [(r, 96) for r in ROWS4] + [(129, i) for i in INNER4 if i != 96]


def mask_pattern(name, rows):
    """bool [rows], or None for "none".  prefix: pseudo-utterances of 50 rows with valid lengths cycling 50, 0, 37, 1 (what the
    model's padded batches look like); tile: rows 128..255 masked."""
    i = torch.arange(rows)
    if name == "none":
        return None
    if name == "ones":
        return torch.ones(rows, dtype=torch.bool)
    if name == "zeros":
        return torch.zeros(rows, dtype=torch.bool)
    if name == "prefix":
        return (i % 50) < torch.tensor([50, 0, 37, 1])[(i // 50) % 4]
    if name == "tile":
        return (i < 128) | (i >= 256)
    raise KeyError(name)


@dataclass(frozen=True)
class Case:
    """One call.  entry: ffn_fused | ffn_prenorm | ffn_prenorm2 | attn_out_ffn | split | split_proj.
    opts (sorted tuple of names): bias1, bias2, rowmajor, noresid (ffn_fused); bias2, stats (ffn_prenorm); stats (ffn_prenorm2);
    stats | norm_f32 | norm_bf16 [+ ln_mask] [+ noout] | qkv (attn_out_ffn); norm_f32 | norm_bf16 [+ ln_mask] (split*)."""
    entry: str
    R: int
    inner: int
    mask: str = "none"
    flags: int = 0
    dim: int = 384
    opts: tuple = ()
    splits: int = 0

    def has(self, o):
        return o in self.opts

    @property
    def label(self):
        return (f"{self.entry}[{','.join(self.opts)}] D={self.dim} R={self.R} inner={self.inner}"
                f"{' x' + str(self.splits) if self.splits else ''} mask={self.mask} flags={self.flags}")


# ------------------------------------------------------------------------------------------------ inputs


def _randn(shape, seed, scale=1.0, mean=0.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + mean


def _bf_round(t):
    return t.to(BF16).float()


@functools.lru_cache(maxsize=None)
def inputs(dim, inner):
    """The fp32 / bf16 operands of every entry at (dim, inner), NROWS rows; bf16 operands are fp32 tensors holding bf16 values."""
    s = 7000 + 13 * dim + inner
    x = _randn((NROWS, dim), s, 0.4, 1.5)
    x[CONST_ROW] = 1.5
    o = _bf_round(_randn((NROWS, dim), s + 1))
    o[CONST_ROW] = 0.0
    return dict(
        x=x, xb=_bf_round(x), resid=_randn((NROWS, dim), s + 2, 0.4, 1.5), o=o,
        wo=_bf_round(_randn((dim, dim), s + 3, dim ** -0.5)), w1=_bf_round(_randn((inner, dim), s + 4, dim ** -0.5)),
        w2=_bf_round(_randn((dim, inner), s + 5, inner ** -0.5)), g=_randn((dim,), s + 6, 0.1, 1.0), b=_randn((dim,), s + 7, 0.1),
        bias1=_randn((inner,), s + 8, 0.1), bias2=_randn((dim,), s + 9, 0.1), fg=_randn((dim,), s + 10, 0.1, 1.0),
        fb=_randn((dim,), s + 11, 0.1), wq=_bf_round(_randn((NQ, dim), s + 12, dim ** -0.5)))


# ------------------------------------------------------------------------------------------------ the formulas


def bf(t):
    """Round float64 values to bf16 (through fp32, as the kernels hold them)."""
    return t.float().to(BF16).to(F64)


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def layer_norm(v, g, b, eps):
    """Biased variance, eps inside the square root."""
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * g.to(F64) + b.to(F64)


def prenorm_ref(v, g, b, eps=EPS, rounded=False, mutant=None):
    ln = layer_norm(v, g, b, 0.0 if mutant == "ln_no_eps" else eps)
    return bf(ln) if rounded else ln


PACK_POS = [(p & 16) | ((p & 4) << 1) | ((p & 8) >> 1) | (p & 3) for p in range(32)]   # position p holds hidden PACK_POS[p]


def pack_perm(inner):
    return torch.tensor([32 * c + PACK_POS[p] for c in range(inner // 32) for p in range(32)])


def hidden_ref(a, w1, bias1=None, rounded=False, mutant=None):
    """gelu_erf(a W1^T + bias1), [rounds, inner]."""
    w1 = w1.to(F64)
    pre = a @ w1.T
    if mutant == "k_half_tail":       # the last chunk's last 8 hidden units summed over the first half of K only
        K = w1.shape[1] // 2
        pre[:, -8:] = a[:, :K] @ w1[-8:, :K].T
    if bias1 is not None:
        pre = pre + bias1.to(F64)
    hid = gelu(pre)
    if rounded:
        hid = bf(hid)
    if mutant == "drop_first_chunk":
        hid[:, :32] = 0.0
    if mutant == "drop_last_chunk":
        hid[:, -32:] = 0.0
    return hid


def second_ref(hid, w2, mutant=None):
    w2 = w2.to(F64)
    if mutant == "w2_pack_order":
        w2 = w2[:, pack_perm(w2.shape[1])]
    return hid @ w2.T


def _mk(mask, rows):
    return torch.ones((rows, 1), dtype=F64) if mask is None else mask.to(F64)[:, None]


def finish_ref(v, resid, mask, flags, mutant=None):
    """MASK_ACC before the residual add, MASK_OUT after it."""
    mk = _mk(mask, v.shape[0])
    acc, out = bool(flags & MASK_ACC), bool(flags & MASK_OUT)
    if mutant == "mask_before_residual" and out:
        acc, out = True, False
    if acc:
        v = v * mk
    if resid is not None:
        v = v + resid
    return v * mk if out else v


def ffn_ref(xb, w1, w2, bias1, bias2, resid, mask, flags, rounded=False, mutant=None):
    """ispk_ffn_bf16: [mask] * (resid + gelu_erf(x W1^T + bias1) W2^T + bias2)."""
    v = second_ref(hidden_ref(xb.to(F64), w1, bias1, rounded, mutant), w2, mutant)
    if bias2 is not None:
        v = v + bias2.to(F64)
    return finish_ref(v, None if resid is None else resid.to(F64), mask, flags, mutant)


def proj_ref(x, o, wo, mask, flags):
    """x1 = x + [mask if MASK_ACC] * (o Wo^T); masked rows of o are not read (they may hold NaN)."""
    o = o.to(F64)
    if flags & MASK_ACC and mask is not None:
        o = torch.where(mask[:, None], o, torch.zeros((), dtype=F64))
    return x.to(F64) + o @ wo.to(F64).T


def stats_ref(out, eps=EPS):
    """(mean, rstd) of rows, float64 [rows, 2]."""
    mean = out.mean(-1)
    return torch.stack([mean, 1.0 / torch.sqrt(((out - mean[:, None]) ** 2).mean(-1) + eps)], 1)


def final_norm_ref(out, fg, fb, mask, ln_mask, bf16, eps=EPS, rounded=False, mutant=None):
    ln = layer_norm(out, fg, fb, eps)
    if ln_mask and mutant != "ln_mask_ignored":
        ln = ln * _mk(mask, out.shape[0])
    return bf(ln) if rounded and bf16 else ln


def qkv_ref(out, g2, b2, wq, eps=EPS, rounded=False, mutant=None):
    """bf16(LN_next(out)) [Wq; Wkv]^T, stored as bf16."""
    h = out if mutant == "qkv_unnormalised" else layer_norm(out, g2, b2, eps)
    q = (bf(h) if rounded else h) @ wq.to(F64).T
    return bf(q) if rounded else q


def split_parts_ref(ln, w1, w2, splits, x1=None, rounded=False, mutant=None):
    """parts[s] = gelu_erf(LN W1_s^T) W2_s^T over hidden units [s inner / splits, (s + 1) inner / splits); x1 (projection form)
    inside parts[0].  float64 [splits, rows, dim]."""
    inner = w1.shape[0]
    n = inner // splits
    parts = []
    for s in range(splits):
        t = s - 1 if mutant == "split_prev_weights" and s > 0 else s
        sl = slice(t * n, (t + 1) * n)
        parts.append(second_ref(hidden_ref(ln, w1[sl], None, rounded, mutant), w2[:, sl], mutant))   # (a chunk mutant: in every split)
    if x1 is not None:
        parts[0] = parts[0] + x1
    return torch.stack(parts)


def combine_ref(x, parts, mask, mutant=None):
    """y = [mask] * (x + sum_s parts[s]), float64."""
    v = parts.to(F64).sum(0)
    if x is not None and mutant != "combine_no_resid":
        v = v + x.to(F64)
    return v * _mk(mask, v.shape[0])


def combine_f32(x, parts, mask, reverse=False):
    """The kernel's sequence of fp32 operations: v = x (0 without x); v += parts[s] in split order; v *= mask.  numpy float32."""
    parts = np.asarray(parts, dtype=np.float32)
    v = np.zeros(parts.shape[1:], dtype=np.float32) if x is None else np.asarray(x, dtype=np.float32).copy()
    for s in (range(parts.shape[0] - 1, -1, -1) if reverse else range(parts.shape[0])):
        v = v + parts[s]
    if mask is not None:
        v = v * np.asarray(mask, dtype=np.float32)[:, None]
    return v


# ------------------------------------------------------------------------------------------------ one case, every output

MUTANTS = ("drop_first_chunk", "drop_last_chunk", "k_half_tail", "w2_pack_order", "mask_before_residual", "ln_no_eps", "ln_of_x_in_proj",
           "stats_of_x1", "last_row_from_prev", "second_tile_from_first", "split_prev_weights", "combine_no_resid",
           "combine_reverse_order", "ln_mask_ignored", "qkv_unnormalised")
PROJ_ENTRIES = ("attn_out_ffn", "split_proj")
SPLIT_ENTRIES = ("split", "split_proj")


def applies(mutant, c: Case) -> bool:
    """Whether `mutant` changes anything an entry of this kind computes (the host test wants a kill per entry it applies to)."""
    e = c.entry
    return {
        "mask_before_residual": e in ("ffn_fused", "ffn_prenorm", "ffn_prenorm2"),
        "ln_no_eps": e != "ffn_fused",
        "ln_of_x_in_proj": e in PROJ_ENTRIES,
        "stats_of_x1": c.has("stats"),
        "split_prev_weights": e in SPLIT_ENTRIES, "combine_no_resid": e == "split", "combine_reverse_order": e in SPLIT_ENTRIES,
        "ln_mask_ignored": c.has("ln_mask"),
        "qkv_unnormalised": c.has("qkv"),
    }.get(mutant, True)


def evaluate(c: Case, rows=None, rounded=False, mutant=None):
    """Every output of the call on the first `rows` rows (default c.R) of the inputs: float64 tensors by name
    (out | y, parts, stats, ln, qkv)."""
    rows = c.R if rows is None else rows
    i = inputs(c.dim, c.inner)
    mask = mask_pattern(c.mask, rows)
    x = i["x"][:rows].to(F64)
    res = {}
    if c.entry == "ffn_fused":
        out = ffn_ref(i["xb"][:rows], i["w1"], i["w2"], i["bias1"] if c.has("bias1") else None, i["bias2"] if c.has("bias2") else None,
                      None if c.has("noresid") else i["resid"][:rows], mask, c.flags, rounded, mutant)
    else:
        x1 = proj_ref(x, i["o"][:rows], i["wo"], mask, c.flags) if c.entry in PROJ_ENTRIES else x
        ln = prenorm_ref(x if mutant == "ln_of_x_in_proj" else x1, i["g"], i["b"], EPS, rounded, mutant)
        if c.entry in SPLIT_ENTRIES:
            proj = c.entry == "split_proj"
            parts = split_parts_ref(ln, i["w1"], i["w2"], c.splits, x1 if proj else None, rounded, mutant)
            res["parts"] = parts
            out = combine_ref(None if proj else x, parts, mask, mutant)
        else:
            v = second_ref(hidden_ref(ln, i["w1"], None, rounded, mutant), i["w2"], mutant)
            if c.has("bias2"):
                v = v + i["bias2"].to(F64)
            # (projection entries: the residual is x1 and MASK_ACC belongs to the projection)
            out = finish_ref(v, x1, mask, c.flags & MASK_OUT if c.entry == "attn_out_ffn" else c.flags, mutant)
    res["y" if c.entry in SPLIT_ENTRIES else "out"] = out
    if c.has("stats"):
        res["stats"] = stats_ref(x1 if mutant == "stats_of_x1" else out)
    for bf16 in (False, True):
        if c.has("norm_bf16" if bf16 else "norm_f32"):
            res["ln"] = final_norm_ref(out, i["fg"], i["fb"], mask, c.has("ln_mask"), bf16, EPS, rounded, mutant)
    if c.has("qkv"):
        res["qkv"] = qkv_ref(out, i["fg"], i["fb"], i["wq"], EPS, rounded, mutant)
    if mutant == "last_row_from_prev" and rows >= 2:
        res = {k: _rows_from(v, k, [rows - 1], [rows - 2]) for k, v in res.items()}
    if mutant == "second_tile_from_first" and rows > 128:
        n = min(rows - 128, 128)
        res = {k: _rows_from(v, k, range(128, 128 + n), range(n)) for k, v in res.items()}
    return res


def _rows_from(v, name, dst, src):
    v = v.clone()
    if name == "parts":
        v[:, list(dst)] = v[:, list(src)]
    else:
        v[list(dst)] = v[list(src)]
    return v


def bound_rows(c: Case) -> int:
    return max(c.R, 128)


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """-> (exact outputs at c.R rows, {output: (max e_round, rms e_round)} taken over bound_rows(c) rows)."""
    n = bound_rows(c)
    exact, rnd = evaluate(c, n), evaluate(c, n, rounded=True)
    e = {}
    for k in exact:
        if k in ("stats", "ln", "qkv"):      # checked against the kernel's own rows
            continue
        d = (rnd[k] - exact[k]).abs()
        if k == "parts":
            e[k] = [(float(d[s].max()), float(d[s].pow(2).mean().sqrt())) for s in range(d.shape[0])]
        else:
            e[k] = (float(d.max()), float(d.pow(2).mean().sqrt()))
    cut = {k: (v[:, :c.R] if k == "parts" else v[:c.R]) for k, v in exact.items()}
    return cut, e


def _ratio(err, allowed):
    return 0.0 if err == 0.0 else (err / allowed if allowed > 0.0 else math.inf)


def value_ratios(got, exact, e_round, what):
    d = (got.to(F64) - exact).abs()
    if bool(torch.isnan(d).any()):
        return {f"{what}.max": math.inf, f"{what}.rms": math.inf}
    return {f"{what}.max": _ratio(float(d.max()), FACTOR * e_round[0]), f"{what}.rms": _ratio(float(d.pow(2).mean().sqrt()), RMS_FACTOR * e_round[1])}


def ratios(c: Case, got: dict) -> dict:
    """Every checked figure of a call's outputs `got` (name -> tensor of c.R rows, any float dtype) divided by what it may be:
    all <= 1 passes.  NaN where none may be counts as inf."""
    exact, e = reference(c)
    i = inputs(c.dim, c.inner)
    mask = mask_pattern(c.mask, c.R)
    main = "y" if c.entry in SPLIT_ENTRIES else "out"
    r = {}
    if main in got:
        r.update(value_ratios(got[main], exact[main], e[main], main))
    if "parts" in got:
        for s in range(c.splits):
            r.update(value_ratios(got["parts"][s], exact["parts"][s], e["parts"][s], f"part{s}"))
    own = got[main].to(F64) if main in got else None
    if "stats" in got:
        want, st = stats_ref(own), got["stats"].to(F64)
        r["stats.mean"] = _nanmax((st[:, 0] - want[:, 0]).abs()) / STATS_MEAN_TOL
        r["stats.rstd"] = _nanmax(((st[:, 1] - want[:, 1]) / want[:, 1]).abs()) / STATS_RSTD_TOL
    if "ln" in got:
        bf16 = c.has("norm_bf16")
        want = final_norm_ref(own, i["fg"], i["fb"], mask, c.has("ln_mask"), bf16)     # (rows not stored: the caller passes the
        r["ln"] = _nanmax((got["ln"].to(F64) - want).abs()) / (LN_TOL[bf16] * max(1.0, float(want.abs().max())))   # storing call's)
    if "qkv" in got:
        want, rnd = qkv_ref(own, i["fg"], i["fb"], i["wq"]), qkv_ref(own, i["fg"], i["fb"], i["wq"], rounded=True)
        r.update(value_ratios(got["qkv"], want, (float((rnd - want).abs().max()), float((rnd - want).pow(2).mean().sqrt())), "qkv"))
    return r


def _nanmax(t):
    return math.inf if bool(torch.isnan(t).any()) else float(t.max()) if t.numel() else 0.0


def masked_rows_are_zero(c: Case, got: dict) -> bool:
    """Wherever the entry masks an output (MASK_OUT rows, the combine pass's y, a row-masked LayerNorm) the masked rows are 0."""
    mask = mask_pattern(c.mask, c.R)
    if mask is None or bool(mask.all()):
        return True
    ok = True
    main = "y" if c.entry in SPLIT_ENTRIES else "out"
    if main in got and (c.entry in SPLIT_ENTRIES or c.flags & MASK_OUT):
        ok &= float(got[main][~mask].abs().max()) == 0.0
    if "ln" in got and c.has("ln_mask"):
        ok &= float(got["ln"][~mask].float().abs().max()) == 0.0
    return ok


# ------------------------------------------------------------------------------------------------ the four-wave kernel's instances


def ffn4_instance(dim, bias1, packed, flags, bias2, resid, prenorm, stats):
    """ffn_launch's dispatch (csrc/ffn.hip) restated: -> (KC, B1, PK, EP, LN, LX) of the ffn_bf16_kernel instance a call runs.
    The hot epilogue is the transformer layer's call: MASK_OUT alone, a residual, no bias2."""
    kc = {256: 4, 384: 6}[dim]
    ep = "hot" if flags == MASK_OUT and resid and not bias2 else "dyn"
    if prenorm:
        assert packed and not bias1 and resid
        return (kc, False, True, ep, bool(stats), True)
    assert not stats
    if not bias1 and packed:
        return (kc, False, True, ep, False, False)
    return (kc, bool(bias1), bool(packed), "dyn", False, False)


def case_instance(c: Case):
    if c.entry == "ffn_prenorm":
        return ffn4_instance(c.dim, False, True, c.flags, c.has("bias2"), True, True, c.has("stats"))
    assert c.entry == "ffn_fused"
    return ffn4_instance(c.dim, c.has("bias1"), not c.has("rowmajor"), c.flags, c.has("bias2"), not c.has("noresid"), False, False)


# The variants of the four-wave entries that every shape of shapes4() runs: (entry, opts, mask, flags)
FFN4_VARIANTS = (
    ("ffn_fused", (), "prefix", MASK_OUT),                          # packed, hot
    ("ffn_fused", ("bias2",), "prefix", MASK_ACC),                  # packed, dynamic epilogue
    ("ffn_fused", ("noresid", "rowmajor"), "none", 0),              # row-major W2 without bias1
    ("ffn_fused", ("bias1", "bias2"), "prefix", MASK_OUT),          # bias1, packed
    ("ffn_fused", ("bias1", "rowmajor"), "prefix", MASK_ACC | MASK_OUT),   # bias1, row-major
    ("ffn_prenorm", (), "prefix", MASK_OUT),                        # pre-norm, hot
    ("ffn_prenorm", ("stats",), "prefix", MASK_OUT),                # pre-norm, hot, statistics
    ("ffn_prenorm", ("bias2",), "prefix", MASK_OUT),                # pre-norm, dynamic (bias2)
    ("ffn_prenorm", ("bias2", "stats"), "none", 0),                 # pre-norm, dynamic, statistics
)


def cases4():
    out = []
    for dim in (256, 384):
        for R, inner in shapes4():
            for entry, opts, mask, flags in FFN4_VARIANTS:
                out.append(Case(entry, R, inner, mask, flags, dim, tuple(sorted(opts))))
    return out


# The variants of the eight-wave entries that every shape runs: (entry, opts); mask and flags come with the shape
FFN2_VARIANTS = (
    ("ffn_prenorm2", ("stats",)), ("attn_out_ffn", ()), ("attn_out_ffn", ("stats",)), ("attn_out_ffn", ("ln_mask", "norm_f32")),
    ("attn_out_ffn", ("ln_mask", "noout", "norm_bf16")), ("attn_out_ffn", ("qkv",)),
)


def cases2():
    out = []
    for entry, opts in FFN2_VARIANTS:
        for R, inner, mask in shapes2(32 if entry == "ffn_prenorm2" else 64):
            fl = MASK_OUT if entry == "ffn_prenorm2" else MASK_ACC | MASK_OUT
            out.append(Case(entry, R, inner, mask, fl, 384, tuple(sorted(opts))))
    return out


def cases_split():
    out = []
    for R, inner, splits in SPLIT_CASES:
        for entry in SPLIT_ENTRIES:
            for opts in ((), ("ln_mask", "norm_bf16"), ("norm_f32",)):
                out.append(Case(entry, R, inner, "prefix", MASK_ACC if entry == "split_proj" else 0, 384, opts, splits))
    return out


def flag_cases():
    """Each mask pattern with 0, MASK_OUT, MASK_ACC and both where the entry permits: at R = 129 / inner 96, `tile` at (257, 160)."""
    out = []
    for mask in MASKS:
        R, inner = (257, 160) if mask == "tile" else (129, 96)
        for fl in FLAG_SETS if mask != "none" else (0,):
            for dim in (256, 384):
                out.append(Case("ffn_fused", R, inner, mask, fl, dim))
                out.append(Case("ffn_prenorm", R, inner, mask, fl, dim, ("stats",)))
            out.append(Case("ffn_prenorm2", R, inner, mask, fl, 384, ("stats",)))
            out.append(Case("attn_out_ffn", R, inner, mask, fl, 384))
            out.append(Case("attn_out_ffn", R, inner, mask, fl, 384, ("stats",)))
            out.append(Case("attn_out_ffn", R, inner, mask, fl, 384, ("qkv",)))
            for lm in ((), ("ln_mask",)) if mask != "none" else ((),):
                out.append(Case("attn_out_ffn", R, inner, mask, fl, 384, tuple(sorted(lm + ("norm_f32",)))))
                out.append(Case("attn_out_ffn", R, inner, mask, fl, 384, tuple(sorted(lm + ("norm_bf16",)))))
        sp = 1      # (3 and 5 chunks: no other split leaves two chunks each)
        for lm in ((), ("ln_mask",)) if mask != "none" else ((),):
            out.append(Case("split", R, inner, mask, 0, 384, tuple(sorted(lm + ("norm_f32",))), sp))
            out.append(Case("split_proj", R, inner, mask, MASK_ACC if mask != "none" else 0, 384, tuple(sorted(lm + ("norm_bf16",))), sp))
        if mask != "none":
            out.append(Case("split_proj", R, inner, mask, 0, 384, (), sp))
    return out


def all_cases():
    seen, out = set(), []
    for c in cases4() + cases2() + cases_split() + flag_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ weight staging


def pack_w2_ref(w2):
    """[dim, inner] -> [inner / 32, dim, 32], position p of a chunk holding hidden unit PACK_POS[p]."""
    dim, inner = w2.shape
    return w2[:, pack_perm(inner)].reshape(dim, inner // 32, 32).permute(1, 0, 2).contiguous()


def chunk_w2_ref(w2):
    dim, inner = w2.shape
    return w2.reshape(dim, inner // 32, 32).permute(1, 0, 2).contiguous()


def chunk_k16_ref(w):
    n, k = w.shape
    return w.reshape(n, k // 16, 16).permute(1, 0, 2).contiguous()
