"""Float64 references of the aligner front end, forward and backward (the aligner half of csrc/aligner.hip and all of
csrc/aligner_bwd.hip), written from each operator's statement in include/ispk.h and the kernels' header comments (no call into
isp_tts_amd), plus the case tables, the seeded inputs, the tolerances and the deliberately wrong references ("mutants") that
tests/test_aligner_reference_host.py and tests/test_gpu_aligner_kernels.py share.

Every `*_ref` takes a `dtype`: float64 is the reference; float32 evaluates THE SAME formula in fp32 torch on the CPU, whose
distance from float64 is the measured rounding noise of an fp32 evaluation (`FP32_NOISE`, re-measured and printed by the host
test), of which a kernel is allowed 8 x, capped at 1e-4 - the margin and the cap of train_kernels_reference.

Remarks on the case tables (where the code decides, the code wins)
  * pad_rows takes the tile kernel when stride_t == 1 and stride_c > 1.  A contiguous [B, C, T] tensor with T = 1 has
    stride_c = 1, so the channel-first inputs here are the time slice [:, :, :T] of a [B, C, T + 3] tensor (a padded batch of
    mels): stride_c = T + 3 at every T, which is what sends (1, 1, 80) to the tile kernel and (65536, 1, 2) to the B > 65535
    fallback.
  * split output: lo = fp16(v' - hi) with v' the CLAMPED value (put_split clamps first), so hi + lo approximates v'.
  * masked_instnorm's eight-fold trip of lane t % 16 runs while its first frame + 112 < n: the tail loops take the frames t with
    t % 16 + 128 (t // 128) + 112 >= n (`tail_frames`), which is what the mutants "instnorm_no_tail" / "_var" drop.
  * the ill-conditioned channel (mean 1e3, deviation 1e-2): an fp32 mean near 1000 cannot be held more finely than 2^-15, a third
    of a percent of such a deviation, whatever the kernel does - no fp32 evaluation of the operator's statement meets 1e-4
    there.  The property the channel pins is that the variance is taken around the mean (E[x^2] - mean^2 loses all of it: x^2 has
    a granularity of 0.06 against a variance of 2.4e-4).  So the channel holds 1000 +- u, alternating over the valid frames (0
    for the last of an odd count), u = 2^-6 = 1.6e-2 while n * 1000 < 2^18 and 2^-5 above: the mean is exactly 1000 and every
    partial sum is exact in fp32 in any order, and a centred variance is exact while an uncentred one is garbage.
  * scores_bwd: d_soft holds NaN in the columns >= text_len (the kernel never reads them); that is what tells
    "scores_bwd_sg_over_L" from the truth, since soft is 0 there.
"""
import numpy as np
import torch

from adaptor_reference import soft_average_ref  # noqa: F401  (the forward the soft-average backward is checked against)
from train_kernels_reference import F64, TOL_CAP, close, rand, rel_err, same_bits  # noqa: F401

F32 = torch.float32
NAN = float("nan")


def _r32(v: float) -> float:
    """A Python scalar as the C entry point receives it (a float argument)."""
    return float(np.float32(v))


def differs(got, want, tol=None) -> bool:
    """True when `got` is not `want`: at all (tol None: an exact check), or by more than tol in max |diff| / max |ref| (NaN counts)."""
    if tol is None:
        return not torch.equal(got, want)
    return not rel_err(got, want) <= tol


def _clamp_len(lengths, lo, hi):
    return torch.as_tensor(lengths).to(torch.int64).clamp(lo, hi)


def tail_frames(n: int):
    """bool [n]: the frames the tail loops of masked_instnorm_kernel take (see the module docstring)."""
    t = torch.arange(n)
    return t % 16 + 128 * (t // 128) + 112 >= n


# ------------------------------------------------------------------------------------------------ pad_rows

SPLIT_MAX = 65504.0


def split_planes(v, clamp=True):
    """fp32 -> (hi, lo) fp16: hi = fp16(v'), lo = fp16(v' - hi), v' = clamp(v, +-65504) (csrc/split.hip's operand format)."""
    v = v.float()
    if clamp:
        v = v.clamp(-SPLIT_MAX, SPLIT_MAX)
    hi = v.half()
    return hi, (v - hi.float()).half()


def split_bound(v):
    """|hi + lo - v'| <= 2^-21 |v'| + 2^-24: hi leaves at most 2^-11 |v'| (or 2^-25 where it is subnormal), lo a 2^-11 of that (or
    half the subnormal spacing 2^-24)."""
    return 2.0 ** -21 * v.double().clamp(-SPLIT_MAX, SPLIT_MAX).abs() + 2.0 ** -24


def pad_rows_ref(x, lengths, mode="f32", dtype=F64, mutant=None):
    """x [B, T, C] (any strides) -> [B, T + 4, C]: frame t < n of utterance b at row t + 2, every other row zero.  The length is
    clamped to n = clamp(len, 0, T).  mode "f32": the copy (in `dtype`); "bf16": rounded to bf16; "split": fp16 planes
    [2, B, T + 4, C] (split_planes)."""
    B, T, C = x.shape
    n = _clamp_len(lengths, 0, T)
    out = torch.zeros((B, T + 4, C), dtype=F32)
    out[:, 2:T + 2] = torch.where((torch.arange(T)[None, :] < n[:, None])[:, :, None], x, torch.zeros(()))
    if mode == "bf16":
        return out.to(torch.bfloat16)
    if mode == "split":
        return torch.stack(split_planes(out, clamp=mutant != "pad_split_no_clamp"))
    return out.to(dtype)


PAD_MODES = [("f32", torch.float32), ("bf16", torch.bfloat16), ("split", torch.float16)]        # (mode, out_dtype of runtime.pad_rows)
PAD_SPECIALS = [1e6, SPLIT_MAX, -SPLIT_MAX, 1e-7]
# (B, T, C) -> layout: "cl" channel-last contiguous, "cl_wide" the column slice [:, :, 8:8 + C] of [B, T, C + 16],
# "cf" channel-first, the time slice [:, :, :T] of [B, C, T + 3]
PAD_CASES = {
    (1, 1, 1): "cl", (2, 28, 4): "cl", (2, 28, 5): "cl", (3, 37, 80): "cl_wide",                 # element-wise kernel
    (2, 28, 32): "cf", (2, 29, 33): "cf", (3, 27, 31): "cf", (1, 1, 80): "cf",                   # tile kernel
    (65536, 1, 2): "cf",                                                                         # B > 65535: element-wise
}
PAD_MUTANTS = ["pad_split_no_clamp"]


def pad_lengths(case):
    """Utterance 0 is always whole (T + 3, clamped, or T in every other case); then 0 (1 in every other case of two), then 1."""
    B, T, C = case
    if B > 64:
        return (torch.arange(B) + 3) % 4                 # 3 (clamped), 0, 1, 2 (clamped), ...
    k = list(PAD_CASES).index(case)
    return torch.tensor([T + 3 if k % 2 == 0 else T, 0 if B == 3 or k % 4 < 2 else 1, 1][:B])


def pad_view(base, case):
    """-> (the tensor runtime.pad_rows takes, channel_first, the same data as [B, T, C])."""
    B, T, C = case
    layout = PAD_CASES[case]
    if layout == "cl":
        return base, False, base
    if layout == "cl_wide":
        v = base[:, :, 8:8 + C]
        return v, False, v
    v = base[:, :, :T]
    return v, True, v.transpose(1, 2)


def pad_inputs(case):
    """-> dict(base, lengths): seeded normal values; 1e6 (clamped by the split mode), +-65504 and 1e-7 planted in the first valid
    elements of utterance 0."""
    B, T, C = case
    layout = PAD_CASES[case]
    seed = 6000 + 10 * list(PAD_CASES).index(case)
    base = rand({"cl": (B, T, C), "cl_wide": (B, T, C + 16), "cf": (B, C, T + 3)}[layout], seed, 3.0)
    x = pad_view(base, case)[2]
    for i, v in enumerate(PAD_SPECIALS):
        t, c = divmod(i, C)
        if t < T:
            x[0, t, c] = v
    return dict(base=base, lengths=pad_lengths(case))


# ------------------------------------------------------------------------------------------------ masked instance norm


def _stats(v, dtype, mutant=None):
    """v [n, C] -> (mean, biased variance) over the n frames."""
    n = v.shape[0]
    keep = (~tail_frames(n)).to(dtype)[:, None]
    mean = (v * keep).sum(0) / n if mutant == "instnorm_no_tail" else v.mean(0)
    d2 = (v - mean) ** 2
    if mutant == "instnorm_no_tail_var":
        d2 = d2 * keep
    var = d2.sum(0) / (max(n - 1, 1) if mutant == "instnorm_var_unbiased" else n)
    return mean, var


def masked_instnorm_ref(y, weight, bias, lengths, eps=1e-5, dtype=F64, mutant=None):
    """y [B, T + 4, C] (row t = frame t) -> out [B, T + 4, C]: per (utterance, channel) mean and biased variance over the n valid
    frames, out row t + 2 = (y[t] - mean) / sqrt(var + eps) * weight + bias for t < n, every other row zero.  The length is
    clamped to n = clamp(len, 1, T)."""
    B, TP, C = y.shape
    n = _clamp_len(lengths, 1, TP - 4)
    out = torch.zeros((B, TP, C), dtype=dtype)
    for b in range(B):
        v = y[b, :int(n[b])].to(dtype)
        mean, var = _stats(v, dtype, mutant)
        out[b, 2:2 + int(n[b])] = (v - mean) / torch.sqrt(var + _r32(eps)) * weight.to(dtype) + bias.to(dtype)
    return out


def masked_instnorm_bwd_ref(y, d_out, weight, lengths, eps=1e-5, dtype=F64, mutant=None):
    """y, d_out [B, T + 4, C] (row t = frame t) -> (d_y like y, d_weight [C], d_bias [C]): with yhat = (y - mean) rstd and
    g = d_out * weight over the n valid frames, d_y[t] = rstd (g_t - mean_t(g) - yhat_t mean_t(g yhat)) for t < n and 0 elsewhere;
    d_weight = sum_b sum_t d_out yhat, d_bias = sum_b sum_t d_out.  The length is clamped to n = clamp(len, 1, T)."""
    B, TP, C = y.shape
    n = _clamp_len(lengths, 1, TP - 4)
    d_y = torch.zeros((B, TP, C), dtype=dtype)
    dw, db = torch.zeros((C,), dtype=dtype), torch.zeros((C,), dtype=dtype)
    w = weight.to(dtype)
    for b in range(B):
        v, go = y[b, :int(n[b])].to(dtype), d_out[b, :int(n[b])].to(dtype)
        mean, var = _stats(v, dtype)
        rstd = 1.0 / torch.sqrt(var + _r32(eps))
        yh = (v - mean) * rstd
        g = go * w
        c2 = 0.0 if mutant == "instnorm_bwd_no_c2" else yh * (g * yh).mean(0)
        d_y[b, :int(n[b])] = rstd * (g - g.mean(0) - c2)
        part = (go * yh).sum(0)
        dw = part if mutant == "instnorm_bwd_param_last_utterance" else dw + part
        db = db + go.sum(0)
    return d_y, dw, db


INSTNORM_MUTANTS = ["instnorm_no_tail", "instnorm_no_tail_var", "instnorm_var_unbiased"]
INSTNORM_BWD_MUTANTS = ["instnorm_bwd_no_c2", "instnorm_bwd_param_last_utterance"]
# (B, T, C) -> lengths.  16 time lanes x 64 channels; the eight-fold trip runs while a lane's frame + 112 < n.
INSTNORM_CASES = {
    (2, 1, 80): (1, 0),             # n = 1 == T (and 0, clamped to 1): variance exactly 0, the output is bias
    (3, 15, 1): (15, 1, 20),        # n = 15 == T; n = 1 < T; 20 clamped to T; one channel
    (3, 16, 64): (16, 15, 1),       # n = 16 == T; 15 < T; one full channel block
    (3, 17, 65): (17, 1, 9),        # n = 17 == T: lane 0 takes two tail frames; a second channel block of one channel
    (3, 112, 63): (112, 16, 17),    # n = 112 == T: tail loop only, 7 frames per lane; 16 and 17 < T
    (2, 113, 160): (113, 112),      # n = 113 == T: lane 0 alone takes the trip; 112 < T; three channel blocks, the last of 32
    (3, 129, 64): (129, 113, 0),    # n = 129 == T: every lane takes the trip, the tail is frame 128 alone; 113 < T
    (3, 300, 80): (300, 129, 17),   # n = 300 == T: two trips; 129 < T
    (2, 301, 1): (300, 15),         # n = 300 < T
}
INSTNORM_MODES = PAD_MODES
INSTNORM_CONST_CHANNEL, INSTNORM_ILL_CHANNEL = 1, 2      # present when C >= 3
# the backward loops are not unrolled: n in {1, 15, 16, 17, 33, 300}
INSTNORM_BWD_CASES = {
    (1, 17, 65): (17,),             # B = 1; a second channel block of one channel
    (3, 33, 64): (33, 16, 1),       # B = 3: the partial sum adds three utterances in order
    (3, 16, 80): (15, 0, 20),       # 0 and 20 clamped to 1 and T
    (1, 300, 1): (300,),
    (2, 9, 260): (9, 5),            # five channel blocks, a second block of instnorm_param_sum_kernel
}


def instnorm_inputs(case, backward=False):
    """-> dict(y, weight, bias, lengths[, d_out]).  Rows t >= n of y (and of d_out), the four scratch rows included, hold NaN.
    Forward, C >= 3: channel 1 is constant (0.75) over its valid frames, channel 2 is 1000 +- u (see the module docstring)."""
    B, T, C = case
    table = INSTNORM_BWD_CASES if backward else INSTNORM_CASES
    lengths = torch.tensor(table[case])
    seed = (7500 if backward else 7000) + 10 * list(table).index(case)
    y = rand((B, T + 4, C), seed, 1.5) + 0.3
    n = _clamp_len(lengths, 1, T)
    for b in range(B):
        nb = int(n[b])
        if not backward and C >= 3:
            y[b, :nb, INSTNORM_CONST_CHANNEL] = 0.75
            u = 2.0 ** -6 if nb * 1000 < 2 ** 18 else 2.0 ** -5
            d = u * (1.0 - 2.0 * (torch.arange(nb) % 2))
            if nb % 2:
                d[-1] = 0.0
            y[b, :nb, INSTNORM_ILL_CHANNEL] = 1000.0 + d
        y[b, nb:] = NAN
    out = dict(y=y, weight=1.0 + 0.3 * rand((C,), seed + 1), bias=rand((C,), seed + 2, 0.5), lengths=lengths)
    if backward:
        d_out = rand((B, T + 4, C), seed + 3)
        for b in range(B):
            d_out[b, int(n[b]):] = NAN
        out["d_out"] = d_out
    return out


# ------------------------------------------------------------------------------------------------ scores

AD = 128                                                     # attention_dim of the aligner
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(AD)))      # as the entry point forms it
PRIOR_CUT = 1e-4
PRIOR_BAND = 1e-4        # a cell is borderline when |prior / 1e-4 - 1| < PRIOR_BAND in float64


def diagonal_prior(text_len, mel_len, M, L, dtype=F64, clamp=True):
    """-> (normalised prior before the cutoff [B, M, L], live [B, M, L]): exp(-(j / tl - m / ml)^2 / (2 * 0.1^2)) for j < tl and
    m < ml, 0 elsewhere, divided by (its row sum + 1e-5).  tl = clamp(text_len, 1, L), ml = clamp(mel_len, 1, M)."""
    tl = _clamp_len(text_len, 1, L) if clamp else torch.as_tensor(text_len)
    ml = _clamp_len(mel_len, 1, M) if clamp else torch.as_tensor(mel_len)
    j, m = torch.arange(L), torch.arange(M)
    live = (j[None, None, :] < tl[:, None, None]) & (m[None, :, None] < ml[:, None, None])
    g = j.to(dtype)[None, None, :] / tl.to(dtype)[:, None, None] - m.to(dtype)[None, :, None] / ml.to(dtype)[:, None, None]
    pe = torch.where(live, torch.exp(-(g * g) / (2 * 0.1 ** 2)), torch.zeros((), dtype=dtype))
    return pe / (pe.sum(-1, keepdim=True) + 1e-5), live


def cut_prior(pr):
    return torch.where(pr < PRIOR_CUT, torch.zeros((), dtype=pr.dtype), pr)


def borderline(text_len, mel_len, M, L, band=PRIOR_BAND):
    """bool [B, M, L]: live cells whose float64 prior sits within `band` (relative) of the cutoff."""
    pr, live = diagonal_prior(text_len, mel_len, M, L)
    return live & ((pr / PRIOR_CUT - 1.0).abs() < band)


def split_bf16_product(q, k, drop=None):
    """The fast path's score product in float64: hi = bf16(v), lo = bf16(v - hi), q.k ~ hi.hi + hi.lo + lo.hi (lo.lo dropped).
    `drop`: "q_lo" / "k_lo" leaves out the cross term with that operand's lo."""
    def parts(v):
        hi = v.float().to(torch.bfloat16).float()
        return hi.double(), (v.float() - hi).to(torch.bfloat16).double()
    qh, ql = parts(q)
    kh, kl = parts(k)
    s = qh @ kh.transpose(1, 2)
    if drop != "k_lo":
        s = s + qh @ kl.transpose(1, 2)
    if drop != "q_lo":
        s = s + ql @ kh.transpose(1, 2)
    return s


def aligner_scores_ref(q, k, text_len, mel_len, M, L, dtype=F64, mutant=None, product=None):
    """q [B, M + 4, 128], k [B, L + 4, 128] (row t = frame / token t) -> (soft, logits), both [B, M, L]:
    logits = log_softmax over ALL L columns of scale * q.k, plus log(prior + 1e-6) with the diagonal prior cut to 0 below 1e-4;
    soft = softmax of the logits over the columns j < tl, 0 elsewhere and in the rows m >= ml.
    tl = clamp(text_len, 1, L), ml = clamp(mel_len, 1, M).  `product`: q.k [B, M, L] from elsewhere (split_bf16_product)."""
    B = q.shape[0]
    qq, kk = q[:, :M].to(dtype), k[:, :L].to(dtype)
    if mutant == "scores_block_swapped":                     # key blocks kb and kb ^ 1 exchanged (where both exist)
        j = torch.arange(L)
        kk = kk[:, torch.where((j ^ 32) < L, j ^ 32, j)]
    s = (qq @ kk.transpose(1, 2) if product is None else product.to(dtype)) * SCALE
    tl, ml = _clamp_len(text_len, 1, L), _clamp_len(mel_len, 1, M)
    keys = torch.arange(L)[None, None, :] < tl[:, None, None]
    rows = torch.arange(M)[None, :, None] < ml[:, None, None]
    ninf = torch.full((), -float("inf"), dtype=dtype)
    if mutant == "scores_lse_over_text_len":
        ls = s - torch.logsumexp(torch.where(keys, s, ninf), dim=-1, keepdim=True)
    else:
        ls = torch.log_softmax(s, dim=-1)
    if mutant == "scores_prior_unclamped_len":
        pr, _ = diagonal_prior(text_len, mel_len, M, L, dtype, clamp=False)
        pr = torch.nan_to_num(pr, nan=0.0, posinf=0.0, neginf=0.0)
    else:
        pr, _ = diagonal_prior(text_len, mel_len, M, L, dtype)
    logits = ls + torch.log(cut_prior(pr) + 1e-6)
    soft = torch.softmax(torch.where(keys, logits, ninf), dim=-1)
    soft = torch.where(keys & rows, soft, torch.zeros((), dtype=dtype))
    if mutant == "scores_row_32_dropped":                    # row 32 of every 64-row tile takes row 31's values
        m = torch.arange(M)
        src = torch.where(m % 64 == 32, m - 1, m)
        soft, logits = soft[:, src], logits[:, src]
    return soft, logits


def aligner_scores_bwd_ref(logits, soft, d_soft, d_logits, text_len, mel_len, scale=SCALE, dtype=F64, mutant=None):
    """The closed form of csrc/aligner_bwd.hip's header.  With A = logits, gs = d_soft, gl = d_logits (either may be None):
    dA_j = gl_j + [j < tl] soft_j (gs_j - sum_{v < tl} soft_v gs_v);  dS_j = scale (dA_j - p_j sum_j dA_j),
    p_j = exp(A_j - log(prior_j + 1e-6)) the softmax over all L columns, the prior recomputed (cut included).
    -> dS [B, M, L] (the kernel also writes the transposed copy dSt[b][j][m] = dS[b][m][j]).
    tl = clamp(text_len, 1, L), ml = clamp(mel_len, 1, M)."""
    B, M, L = logits.shape
    A, S = logits.to(dtype), soft.to(dtype)
    tl = _clamp_len(text_len, 1, L)
    keys = torch.arange(L)[None, None, :] < tl[:, None, None]
    zero = torch.zeros((), dtype=dtype)
    dA = torch.zeros((B, M, L), dtype=dtype) if d_logits is None else d_logits.to(dtype).clone()
    if d_soft is not None:
        gs = d_soft.to(dtype)
        if mutant == "scores_bwd_sg_over_L":
            sg = (S * gs).sum(-1, keepdim=True)
        else:
            sg = torch.where(keys, S * gs, zero).sum(-1, keepdim=True)
        dA = dA + torch.where(keys, S * (gs - sg), zero)
    pr, _ = diagonal_prior(text_len, mel_len, M, L, dtype)
    p_all = torch.exp(A - torch.log(cut_prior(pr) + 1e-6))
    tot = dA.sum(-1, keepdim=True)
    if mutant == "scores_bwd_no_logsoftmax_term":
        return _r32(scale) * dA
    return _r32(scale) * (dA - p_all * tot)


SCORES_MUTANTS = ["scores_block_swapped", "scores_lse_over_text_len", "scores_prior_unclamped_len", "scores_row_32_dropped"]
SCORES_BWD_MUTANTS = ["scores_bwd_sg_over_L", "scores_bwd_no_logsoftmax_term"]
# (B, M, L) -> (text_len, mel_len).  NB = ceil(L / 32) key blocks in registers; a wave owns 32 mel rows, a workgroup 64.
SCORES_CASES = {
    (2, 31, 1): ((1, 0), (31, 0)),                    # NB 1: one key - the LDS is the two transpose patches; lengths 0, clamped
    (2, 1, 31): ((31, 17), (1, 1)),                   # NB 1, scalar stores; M = 1
    (3, 32, 32): ((32, 37, 1), (32, 39, 20)),         # NB 1, vector stores; wave 1 has no live row; lengths above, clamped
    (2, 33, 33): ((33, 32), (33, 7)),                 # NB 2: block 1 has one live key; wave 1 has one live row; q a batch slice
    (2, 64, 64): ((64, 40), (71, 33)),                # NB 2 full; M + 7 clamped; scores up to +-80
    (2, 65, 65): ((65, 0), (65, 64)),                 # NB 3; a second workgroup with one live row
    (2, 130, 100): ((100, 57), (130, 77)),            # NB 4: the bench's L; three workgroups
    (2, 33, 129): ((129, 100), (33, 0)),              # NB 5
    (2, 65, 160): ((165, 130), (65, 40)),             # NB 5: the largest L at which two workgroups share a CU; L + 5 clamped
    (2, 31, 161): ((161, 33), (31, 1)),               # NB 6
    (2, 32, 193): ((193, 150), (32, 9)),              # NB 7
    (2, 64, 226): ((226, 101), (64, 50)),             # NB 8, L % 4 == 2
    (2, 1, 257): ((257, 200), (1, 1)),                # NB 9; M = 1
    (2, 130, 289): ((289, 270), (130, 100)),          # NB 10
    (3, 65, 320): ((320, 325, 1), (65, 0, 72)),       # NB 10: the documented maximum, 160 KiB of dynamic LDS
}
SCORES_Q_SLICE = (2, 33, 33)        # q is the batch slice [::2] of a [2 B, M + 4, 128] tensor: q_stride_b = 2 (M + 4) 128
SCORES_BIG = (2, 64, 64)            # q scaled so that the largest |scale q.k| is 80
SCORES_PLANT = 1.0 + 0.45 * 2.0 ** -7   # bf16 hi = 1, lo = 0.45 * 2^-7: the largest lo a value can carry, the same sign in every dim
# one wave per (b, m) row, four rows per workgroup, columns strided by 64
SCORES_BWD_CASES = {
    (1, 1, 1): ((1,), (1,)),                          # B M = 1
    (2, 2, 64): ((64, 0), (2, 5)),                    # B M = 4: one full workgroup; lengths 0 and above M
    (1, 4, 63): ((70,), (3,)),                        # B M = 4; L4 > L; text_len above L; row 3 is past mel_len
    (1, 5, 65): ((40,), (5,)),                        # B M = 5: a second workgroup with one live wave; L4 > L, M4 > M
    (5, 1, 130): ((130, 1, 0, 77, 129), (1, 1, 0, 1, 3)),   # B M = 5 over five utterances; M4 > M
    (1, 5, 320): ((320,), (4,)),                      # five trips per lane
    (3, 33, 65): ((65, 33, 64), (33, 20, 0)),         # rows >= mel_len in two utterances
}
SCORES_BWD_MODES = ["soft", "logits", "both"]


def scores_inputs(case):
    """-> dict(q, k, wide, text_len, mel_len): normal q [B, M + 4, 128], k [B, L + 4, 128] whose four scratch rows hold NaN.  Row
    0 of q and key 0 of k hold SCORES_PLANT in every dim (a coherent bf16 lo term: what a lost cross term of the fast path shows
    on).  `q` is a view of `wide` where that is not None."""
    B, M, L = case
    seed = 8000 + 10 * list(SCORES_CASES).index(case)
    q, k = rand((B, M + 4, AD), seed), rand((B, L + 4, AD), seed + 1)
    q[:, 0], k[:, 0] = SCORES_PLANT, SCORES_PLANT
    if case == SCORES_BIG:
        q[:, :M] *= 80.0 / float((q[:, :M].double() @ k[:, :L].double().transpose(1, 2)).abs().max() * SCALE)
    q[:, M:], k[:, L:] = NAN, NAN
    wide = None
    if case == SCORES_Q_SLICE:
        wide = rand((2 * B, M + 4, AD), seed + 2)
        wide[::2] = q
        q = wide[::2]
    tl, ml = SCORES_CASES[case]
    return dict(q=q, k=k, wide=wide, text_len=torch.tensor(tl), mel_len=torch.tensor(ml))


def scores_checked(case, table=None):
    """-> (cells [B, M, L], rows [B, M]): what the comparison with float64 keeps - every cell but the borderline ones (logits),
    every row without one (soft, dS)."""
    B, M, L = case
    tl, ml = (table or SCORES_CASES)[case]
    bl = borderline(torch.tensor(tl), torch.tensor(ml), M, L)
    return ~bl, ~bl.any(-1)


def live_rows(case, table=None):
    B, M, L = case
    ml = _clamp_len((table or SCORES_CASES)[case][1], 1, M)
    return torch.arange(M)[None, :] < ml[:, None]


def scores_bwd_inputs(case, mode):
    """-> dict(logits, soft, d_soft, d_logits, text_len, mel_len): logits and soft are the float64 forward of seeded q, k rounded
    to fp32; d_soft holds NaN in the columns >= tl."""
    B, M, L = case
    seed = 8500 + 10 * list(SCORES_BWD_CASES).index(case)
    tl, ml = (torch.tensor(v) for v in SCORES_BWD_CASES[case])
    q, k = rand((B, M + 4, AD), seed), rand((B, L + 4, AD), seed + 1)
    soft, logits = aligner_scores_ref(q, k, tl, ml, M, L)
    d_soft = d_logits = None
    if mode in ("soft", "both"):
        d_soft = rand((B, M, L), seed + 2)
        d_soft[(torch.arange(L)[None, :] >= _clamp_len(tl, 1, L)[:, None])[:, None, :].expand(B, M, L)] = NAN
    if mode in ("logits", "both"):
        d_logits = rand((B, M, L), seed + 3)
    return dict(logits=logits.float(), soft=soft.float(), d_soft=d_soft, d_logits=d_logits, text_len=tl, mel_len=ml, q=q, k=k)


def scores_bwd_err(got, want, i) -> float:
    """max |diff| / max |ref| - except at L = 1, where the reference is identically 0 (the softmax of one column is constant):
    there the unit is scale * max |cotangent|, the size of the two terms that cancel."""
    if want.shape[-1] > 1:
        return rel_err(got, want)
    unit = SCALE * max(float(torch.nan_to_num(g, nan=0.0).abs().max()) for g in (i["d_soft"], i["d_logits"]) if g is not None)
    return float((got.detach().cpu().double() - want.detach().cpu().double()).abs().max()) / unit


# ---- the fast path's bound (derived; see tests/test_gpu_aligner_kernels.py's docstring)

U = 2.0 ** -23


def fast_transcendental_term(q, k, M, L) -> float:
    """What v_exp_f32 / v_log_f32 and the fp32 `* log2(e)` scaling may add to a logit, at the largest arguments of this case.
    exp(x) = v_exp(x * log2e): the product's rounding and the constant's move the exponent by at most 2^-23 |x| log2e, the result
    by a factor 2^-23 |x|; v_exp_f32 itself is good to 1 ulp = 2^-23: e(x) = 2^-23 (1 + |x|) relative.
    log(y) = v_log(y) * ln2: 1 ulp of the log2, the product's rounding and the constant's: 2^-22 |log y| absolute.
    lse = rmax + log(sum exp(s - rmax)): the sum's relative error e(A), A = max |s - rmax|, is an absolute error of the log;
    plus 2^-22 log L.  log(prior + 1e-6): the prior is a quotient of such exponentials with |x| < 50 (relative 2 e(50)), and
    |log| <= log(1e6) = 13.82."""
    s = (q[:, :M].double() @ k[:, :L].double().transpose(1, 2)) * SCALE
    A = float((s.max(-1, keepdim=True).values - s).max())
    e = lambda x: U * (1.0 + abs(x))      # noqa: E731
    return e(A) + 2 * U * np.log(max(L, 2)) + 2 * e(50.0) + 2 * U * 13.82


def fast_logit_bound(q, k, M, L, fp32_tol_abs: float):
    """[B, M, L]: fp32 tolerance + 2 * 2^-16 * scale * (|q_m| . |k_j| + max_j' |q_m| . |k_j'|) + the transcendental term."""
    P = (q[:, :M].double().abs() @ k[:, :L].double().abs().transpose(1, 2)) * SCALE
    return fp32_tol_abs + 2 * 2.0 ** -16 * (P + P.max(-1, keepdim=True).values) + fast_transcendental_term(q, k, M, L)


# ------------------------------------------------------------------------------------------------ soft averages, backward


def soft_average_bwd_ref(attn, pitch, energy, d_feats, text_len, dtype=F64, prior=None, mutant=None):
    """d attn [B, M, L] of feats[b][l][1 + k] = mask_l N_k[l] / D[l], N_k = sum_m x_k[m] A[m][l], D = sum_m A[m][l] + 1e-5:
    dA[m][l] = mask_l sum_k g_k[l] (x_k[m] - N_k[l] / D[l]) / D[l], mask_l = l < text_len (taken as given: 0 masks every column);
    added to `prior` when that is given (accumulate = 1)."""
    A = attn.to(dtype)
    B, M, L = A.shape
    D = A.sum(1) + (0.0 if mutant == "sa_bwd_no_eps" else 1e-5)                     # [B, L]
    g = d_feats.to(dtype)
    dA = torch.zeros((B, M, L), dtype=dtype)
    for col, x in ((1, pitch), (2, energy)):
        xx = x.to(dtype)
        N = (xx[:, None, :] @ A)[:, 0]                                              # [B, L]
        dA = dA + g[:, None, :, col] * (xx[:, :, None] - (N / D)[:, None, :]) / D[:, None, :]
    if mutant != "sa_bwd_mask_ignored":
        mask = torch.arange(L)[None, :] < torch.as_tensor(text_len)[:, None]
        dA = torch.where(mask[:, None, :], dA, torch.zeros((), dtype=dtype))
    return dA if prior is None else prior.to(dtype) + dA


SA_BWD_MUTANTS = ["sa_bwd_no_eps", "sa_bwd_mask_ignored"]
# (B, M, L) -> text_len.  Column pass: one wave per (b, l), four columns per workgroup, frames strided by 64; second pass: 256
# elements per workgroup
SA_BWD_CASES = {
    (1, 1, 4): (4,),                    # M = 1: one frame, lane 0 alone
    (1, 63, 4): (3,),                   # B L = 4: one full workgroup of columns; 252 elements
    (1, 64, 4): (4,),                   # exactly 256 elements
    (1, 257, 1): (1,),                  # B L = 1; 257 elements: a second workgroup of one; five frames for lane 0
    (1, 65, 5): (0,),                   # B L = 5: a second column workgroup with one live wave; text_len 0: everything masked
    (5, 130, 1): (1, 0, 1, 1, 0),       # B L = 5 over five utterances; three frames for lanes 0 and 1
    (2, 130, 7): (7, 4),
}


def sa_bwd_inputs(case):
    """softmax alignments with one all-zero text column inside text_len (L > 1: D = 1e-5 there; its d_feats are scaled by 1e-5, so
    that its gradient x g / 1e-5 is of the size of the others and max |ref| measures every column), d_feats [B, L, 3], the seeded
    values `prior` an accumulating call adds to."""
    B, M, L = case
    seed = 9000 + 10 * list(SA_BWD_CASES).index(case)
    attn = torch.softmax(rand((B, M, L), seed, 3.0 if M > 1 else 0.5), dim=-1)     # (M = 1: x - N / D cancels to x 1e-5 / D)
    zero_col = 1 if L > 1 else None
    if zero_col is not None:
        attn[:, :, zero_col] = 0.0
    d_feats = rand((B, L, 3), seed + 3)
    if zero_col is not None:
        d_feats[:, zero_col] *= 1e-5
    return dict(attn=attn, pitch=rand((B, M), seed + 1, 0.5) + 1.0, energy=rand((B, M), seed + 2), d_feats=d_feats,
                text_len=torch.tensor(SA_BWD_CASES[case]), prior=rand((B, M, L), seed + 4), zero_col=zero_col)


# ------------------------------------------------------------------------------------------------ fp32 noise
# max over the case tables of rel_err(fp32 evaluation on the CPU, float64 reference), per kernel output: measured by
# tests/test_aligner_reference_host.py::test_fp32_noise_table (which prints the per-case figures and fails when an entry here
# is below what it measures, or more than a factor 4 above).  torch's sums and the BLAS behind `@` choose their order by CPU and
# thread count, so the figures differ between machines (adaptor_reference.FP32_NOISE saw a factor 2.2): each entry is 1.4 x
# what was measured where this was written.  A kernel is allowed 8 x its figure, and never more than 1e-4.
FP32_NOISE = {
    "instnorm.out": 2.2e-7,
    "instnorm_bwd.d_y": 1.0e-6, "instnorm_bwd.d_weight": 2.8e-7, "instnorm_bwd.d_bias": 3.0e-7,
    "scores.logits": 1.1e-6, "scores.soft": 1.9e-6,
    "scores_bwd.dS": 4.8e-7,
    "soft_average_bwd.dA": 7.9e-7,
}
PRIOR_FP32_DISTANCE = 3.8e-6      # max relative distance of the fp32 prior from float64 over the cells >= 1e-5 of SCORES_CASES


def tol(key: str) -> float:
    return min(8.0 * FP32_NOISE[key], TOL_CAP)


def measure_fp32_noise() -> dict:
    """key -> {case label: rel_err of the fp32 evaluation} over every case of every kernel whose tolerance is measured (the
    borderline cells and rows of the prior's cutoff left out, as the GPU test leaves them out)."""
    out: dict = {k: {} for k in FP32_NOISE}
    for case in INSTNORM_CASES:
        i = instnorm_inputs(case)
        out["instnorm.out"][f"{case}"] = rel_err(masked_instnorm_ref(**i, dtype=F32), masked_instnorm_ref(**i))
    for case in INSTNORM_BWD_CASES:
        i = instnorm_inputs(case, backward=True)
        i.pop("bias")
        for name, a, b in zip(("d_y", "d_weight", "d_bias"), masked_instnorm_bwd_ref(**i, dtype=F32), masked_instnorm_bwd_ref(**i)):
            out[f"instnorm_bwd.{name}"][f"{case}"] = rel_err(a, b)
    for case in SCORES_CASES:
        B, M, L = case
        i = scores_inputs(case)
        args = (i["q"], i["k"], i["text_len"], i["mel_len"], M, L)
        (s32, l32), (s64, l64) = aligner_scores_ref(*args, dtype=F32), aligner_scores_ref(*args)
        cells, rows = scores_checked(case)
        out["scores.logits"][f"{case}"] = rel_err(l32[cells], l64[cells])
        out["scores.soft"][f"{case}"] = rel_err(s32[rows], s64[rows])
    for case in SCORES_BWD_CASES:
        _, rows = scores_checked(case, SCORES_BWD_CASES)
        for mode in SCORES_BWD_MODES:
            i = scores_bwd_inputs(case, mode)
            args = (i["logits"], i["soft"], i["d_soft"], i["d_logits"], i["text_len"], i["mel_len"])
            out["scores_bwd.dS"][f"{case} {mode}"] = scores_bwd_err(aligner_scores_bwd_ref(*args, dtype=F32)[rows],
                                                                     aligner_scores_bwd_ref(*args)[rows], i)
    for case in SA_BWD_CASES:
        i = sa_bwd_inputs(case)
        args = (i["attn"], i["pitch"], i["energy"], i["d_feats"], i["text_len"])
        out["soft_average_bwd.dA"][f"{case}"] = rel_err(soft_average_bwd_ref(*args, dtype=F32), soft_average_bwd_ref(*args))
    return out


def measure_prior_fp32_distance() -> float:
    """max over SCORES_CASES and the cells with a prior >= 1e-5 of |prior_fp32 / prior_float64 - 1|."""
    worst = 0.0
    for (B, M, L), (tl, ml) in SCORES_CASES.items():
        p64, live = diagonal_prior(torch.tensor(tl), torch.tensor(ml), M, L)
        p32, _ = diagonal_prior(torch.tensor(tl), torch.tensor(ml), M, L, dtype=F32)
        sel = live & (p64 >= 1e-5)
        if bool(sel.any()):
            worst = max(worst, float((p32.double()[sel] / p64[sel] - 1.0).abs().max()))
    return worst
