"""Float64 references of the adaptor and between-stack kernels (csrc/glue.hip and the non-aligner half of csrc/aligner.hip),
written from each operator's statement in include/ispk.h (no call into isp_tts_amd), plus the case tables, the seeded inputs,
the tolerances and the deliberately wrong references ("mutants") that tests/test_adaptor_reference_host.py and
tests/test_gpu_adaptor_kernels.py share.

Every `*_ref` takes a `dtype`: float64 is the reference; float32 evaluates THE SAME formula in fp32 torch on the CPU.  That
evaluation serves twice: where the operator is a fixed sequence of single roundings (flow_mix, flow_euler, flow_finish's pred,
infer_features' feature columns and target durations, embed_tokens) the kernel must equal it bit for bit, and everywhere else
its distance from float64 is the measured rounding noise of an fp32 evaluation (`FP32_NOISE`, re-measured and printed by the
host test), of which a kernel is allowed 8 x, capped at 1e-4 - the margin and the cap of train_kernels_reference.

The case tables are the issue's.  One remark on SA_CASES: the tail loop of soft_average_kernel takes the frames m with
m % 16 + 128 (m // 128) + 112 >= M (lane m % 16 runs the eight-fold trip only while its first frame + 112 < M), which is what
the mutant "sa_no_tail" drops; "sa_no_tail_after" drops the frames m >= 112 + (M - 112) % 16 instead.  Both are killed.
"""
import numpy as np
import torch

from train_kernels_reference import (F64, TOL_CAP, close, rand, rel_err, same_bits, time_embedding_fwd,  # noqa: F401
                                     time_features, time_inputs)

F32 = torch.float32


def _r32(v: float) -> float:
    """A Python scalar as the C entry point receives it (a float argument)."""
    return float(np.float32(v))


def _lens(B: int, L: int) -> list:
    """Lengths in [0, L]: L alone for B = 1, else L, 0 and a spread."""
    return [L] if B == 1 else [L, 0] + [(3 * b + 1) % (L + 1) for b in range(2, B)]


def _len_mask(lens, L):
    return torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]


def differs(got, want, tol=None) -> bool:
    """True when `got` is not `want`: at all (tol None: an exact check), or by more than tol in max |diff| / max |ref| (NaN counts)."""
    if tol is None:
        return not torch.equal(got, want)
    return not rel_err(got, want) <= tol


# ------------------------------------------------------------------------------------------------ length regulator


def dec_len_ref(dur, max_len=-1):
    """(fp32 sum over ALL L durations + 0.5) truncated, clamped to max_len when max_len >= 0.  int64 [B]."""
    s = dur.sum(1).float() if dur.dtype == torch.int64 else dur.float().sum(1)
    dl = (s + 0.5).long()
    return dl.clamp(max=max_len) if max_len >= 0 else dl


def soft_path_ref(dur, M, dec_len, enc_len, dtype=F64, mask_tokens=True, mask_frames=True):
    """A [B, M, L]: A[b][y][t] = P[t][y] = clamp(cum[t+1] - y, 0, 1) - clamp(cum[t] - y, 0, 1), cum[t] = sum_{u < t} dur[u],
    masked by t < enc_len[b] (None: L) and y < dec_len[b]."""
    B, L = dur.shape
    cum = torch.cat([torch.zeros((B, 1), dtype=dtype), torch.cumsum(dur.to(dtype), 1)], 1)
    ramp = (cum[:, :, None] - torch.arange(M, dtype=dtype)).clamp(0.0, 1.0)          # [B, L + 1, M]
    P = ramp[:, 1:] - ramp[:, :-1]
    if mask_tokens and enc_len is not None:
        P = P * _len_mask(enc_len, L).to(dtype)[:, :, None]
    if mask_frames:
        P = P * _len_mask(dec_len, M).to(dtype)[:, None, :]
    return P.transpose(1, 2)


def length_regulate_ref(x, dur, alignment, M, max_len=-1, enc_len=None, dtype=F64):
    """-> out [B, M, D] = A @ x over every row (rows past dec_len included: with an alignment nothing masks them), dec_len
    int64 [B], dec_mask bool [B, M].  A = alignment, or the soft path of the fp32 durations."""
    dl = dec_len_ref(dur, max_len)
    A = alignment.to(dtype) if alignment is not None else soft_path_ref(dur, M, dl, enc_len, dtype)
    return A @ x.to(dtype), dl, _len_mask(dl, M)


LR_MUTANTS = ["lr_drop_last_chunk", "lr_no_enc_len_mask", "lr_no_max_len_clamp", "lr_no_dec_len_mask", "lr_swap_tile_halves",
              "lr_second_feature_group"]


def length_regulate_mutant(name, x, dur, alignment, M, max_len=-1, enc_len=None, dtype=F64):
    B, L, D = x.shape
    dl = dec_len_ref(dur, -1 if name == "lr_no_max_len_clamp" else max_len)
    A = alignment.to(dtype) if alignment is not None else soft_path_ref(
        dur, M, dl, enc_len, dtype, mask_tokens=name != "lr_no_enc_len_mask", mask_frames=name != "lr_no_dec_len_mask")
    xx = x.to(dtype)
    if name == "lr_drop_last_chunk" and L % 16:          # the last, partial chunk of 16 tokens
        A = A.clone()
        A[:, :, L - L % 16:] = 0
    if name == "lr_second_feature_group":                # a wave's second 128-feature group in place of the first
        xx = xx.clone()
        xx[..., :128] = xx[..., 128:256]
    out = A @ xx
    if name == "lr_swap_tile_halves":                    # rows 32..63 of every 64-frame tile against rows 0..31
        y = torch.arange(M)
        out = out[:, torch.where((y ^ 32) < M, y ^ 32, y)]
    return out, dl, _len_mask(dl, M)


# (B, M, L, D).  A workgroup owns 64 frames, the token axis runs in chunks of 16, NT = D / 128.
LR_CASES = [(2, 1, 1, 256), (1, 63, 15, 256), (2, 64, 16, 256), (3, 65, 17, 384), (2, 128, 48, 384), (2, 130, 33, 384)]
LR_MODES = ["align_i64", "align_i64_sum", "align_f32", "soft", "soft_enc"]
LR_ENTRIES = [("fp32", False), ("split_bf16", True), ("split_f16", "f16")]      # (label, `split_bf16` of runtime.length_regulate)
# per case: max_len; per utterance the range of its durations in quarters (fp32 durations = q / 4 in [0, 6], int64 durations
# = ceil(q / 4)); enc_len of the "soft_enc" mode; whether x is the column slice [:, :, 8:8 + D] of a [B, L, D + 16] tensor
LR_SETUP = {
    (2, 1, 1, 256):    dict(max_len=-1, quarters=[(12, 12), (0, 0)], enc_len=[1, 0], wide=False),       # sum 3 > M, unclamped; all 0
    (1, 63, 15, 256):  dict(max_len=40, quarters=[(8, 24)], enc_len=[9], wide=True),                    # max_len < sum, < M
    (2, 64, 16, 256):  dict(max_len=64, quarters=[(16, 24), (0, 16)], enc_len=[16, 0], wide=False),     # clamped to M / below M
    (3, 65, 17, 384):  dict(max_len=-1, quarters=[(16, 24), (0, 0), (4, 16)], enc_len=[17, 0, 16], wide=False),
    (2, 128, 48, 384): dict(max_len=100, quarters=[(8, 16), (0, 12)], enc_len=[48, 0], wide=True),      # max_len < sum, < M
    (2, 130, 33, 384): dict(max_len=130, quarters=[(12, 24), (0, 24)], enc_len=[0, 33], wide=False),
}


def lr_inputs(case, mode, exact=True):
    """-> dict(x, wide, dur, alignment, M, max_len, enc_len).  `exact`: integer alignments in [-4, 4], integer x in [-64, 64] and
    durations that are multiples of 0.25 - every product, sum, ramp and weight is exact in fp32 (and in split bf16 / fp16 terms) in
    any order.  Otherwise (alignment modes only) softmax alignments and normal x.  `x` is a view of `wide` where that is not None."""
    B, M, L, D = case
    s = LR_SETUP[case]
    seed = 1000 + 10 * LR_CASES.index(case)
    g = torch.Generator().manual_seed(seed)
    q = torch.stack([torch.randint(lo, hi + 1, (L,), generator=g) for lo, hi in s["quarters"]])
    xv = torch.randint(-64, 65, (B, L, D), generator=g).float() if exact else rand((B, L, D), seed + 1)
    wide = None
    if s["wide"]:
        wide = rand((B, L, D + 16), seed + 2)
        wide[:, :, 8:8 + D] = xv
        xv = wide[:, :, 8:8 + D]
    alignment = enc_len = None
    if mode.startswith("align"):
        alignment = (torch.randint(-4, 5, (B, M, L), generator=g).float() if exact
                     else torch.softmax(rand((B, M, L), seed + 3, 3.0), dim=-1))
    else:
        assert exact
    if mode == "soft_enc":
        enc_len = torch.tensor(s["enc_len"])
    dur = q.float() * 0.25
    if mode.startswith("align_i64"):
        dur = (q + 3) // 4
        if mode == "align_i64_sum":
            dur = dur.sum(1, keepdim=True)
    return dict(x=xv, wide=wide, dur=dur, alignment=alignment, M=M, max_len=s["max_len"], enc_len=enc_len)


def lr_bf16_bound(alignment, x):
    """The header's figure for the bf16 entry, per element: 2^-16 (|A| @ |x|).  A bf16 lo term leaves a residual of at most 2^-18
    of its operand, the dropped lo-lo product is below 2^-18 of the product: three such terms stay under 2^-16."""
    return 2.0 ** -16 * (alignment.double().abs() @ x.double().abs())


# ------------------------------------------------------------------------------------------------ soft averages


def sa_tail_frames(M):
    """bool [M]: the frames soft_average_kernel's tail loop takes (see the module docstring)."""
    m = torch.arange(M)
    return m % 16 + 128 * (m // 128) + 112 >= M


def soft_average_ref(attn, pitch, energy, duration, text_len, dtype=F64, mutant=None):
    """feats [B, L, 3] = { log1p(dur) (0 without durations), mask * sum_m pitch[m] A[m][l] / (sum_m A[m][l] + 1e-5), same for
    energy }, mask = l < text_len[b]."""
    A = attn.to(dtype)
    B, M, L = A.shape
    if mutant == "sa_no_tail":
        A = A * (~sa_tail_frames(M)).to(dtype)[None, :, None]
    if mutant == "sa_no_tail_after" and M > 112:
        A = A * (torch.arange(M) < 112 + (M - 112) % 16).to(dtype)[None, :, None]
    col = A.sum(1) + 1e-5
    mk = torch.ones((B, L), dtype=dtype) if mutant == "sa_no_text_len" else _len_mask(text_len, L).to(dtype)
    pt = (pitch.to(dtype)[:, None, :] @ A)[:, 0] / col * mk
    et = (energy.to(dtype)[:, None, :] @ A)[:, 0] / col * mk
    ld = torch.zeros((B, L), dtype=dtype) if duration is None else torch.log1p(duration.to(dtype))
    return torch.stack([ld, pt, et], dim=-1)


SA_MUTANTS = ["sa_no_tail", "sa_no_tail_after", "sa_no_text_len"]
# (B, M, L): 16 frame lanes; the eight-fold trip runs while a lane's frame + 112 < M; 64 text columns per workgroup
SA_CASES = [(2, 1, 1), (2, 15, 5), (3, 17, 65), (2, 112, 64), (2, 113, 63), (2, 129, 64), (1, 300, 130)]


def sa_inputs(case):
    """softmax alignments with one all-zero text column (L > 1), text_len with 0 and L, int64 durations with zeros."""
    B, M, L = case
    seed = 2000 + 10 * SA_CASES.index(case)
    attn = torch.softmax(rand((B, M, L), seed, 3.0), dim=-1)
    zero_col = L // 2 if L > 1 else None
    if zero_col is not None:
        attn[:, :, zero_col] = 0.0
    g = torch.Generator().manual_seed(seed + 3)
    dur = torch.randint(0, 7, (B, L), generator=g)
    dur[:, 0] = 0
    text_len = torch.tensor(_lens(B, L) if B > 1 else [max(1, (3 * L) // 5)])
    return dict(attn=attn, pitch=rand((B, M), seed + 1, 0.5) + 1.0, energy=rand((B, M), seed + 2), duration=dur, text_len=text_len,
                zero_col=zero_col)


# ------------------------------------------------------------------------------------------------ flow-matching algebra


def flow_mix_ref(x0, x1, t, sigma, dtype=F64):
    """x_t = (1 - (1 - sigma) t_b) x0 + t_b x1 ; flow = x1 - (1 - sigma) x0; 1 - sigma formed in double, then one rounding per
    operation in the order written."""
    x0, x1, tt = x0.to(dtype), x1.to(dtype), t.to(dtype)[:, None, None]
    s = 1 - sigma
    return (1 - s * tt) * x0 + tt * x1, x1 - s * x0


FLOW_MUTANTS = ["flow_first_1024", "flow_no_floor", "flow_no_row_mask"]


def flow_finish_ref(raw, flow, x0, mask, dtype=F64, mutant=None):
    """pf = raw * mask ; pred = (x0 + pf) * mask ; duration = max(exp(pred[..., 0]) - 1, 0) ; ratio[b] = sum over valid (l, c) of
    (pf - flow)^2 / max(C * valid_l, 1e-5) ; loss = mean_b ratio.  -> pred [B, L, C], duration [B, L], ratio [B], loss 0-d."""
    raw, flow, x0 = raw.to(dtype), flow.to(dtype), x0.to(dtype)
    B, L, C = raw.shape
    m3 = mask.to(dtype)[:, :, None]
    pf = raw * m3
    pred = (x0 + pf) * m3
    dur = torch.clamp(torch.exp(pred[..., 0]) - 1.0, min=0.0)
    num = ((pf - flow) ** 2 * m3).sum((1, 2))
    den = C * mask.to(dtype).sum(1)
    ratio = num / (den if mutant == "flow_no_floor" else den.clamp(min=1e-5))
    loss = (ratio[:1024] if mutant == "flow_first_1024" else ratio).sum() / B
    return pred, dur, ratio, loss


def flow_head_ref(y, gamma, beta, eps, W, bias, flow, x0, mask, dtype=F64, mutant=None):
    """LayerNorm over 256 with its row mask (masked rows are 0 whatever they hold), the 256 -> 3 linear, then flow_finish_ref."""
    y = y.to(dtype)
    yc = y - y.mean(-1, keepdim=True)
    h = yc / torch.sqrt((yc * yc).mean(-1, keepdim=True) + _r32(eps)) * gamma.to(dtype) + beta.to(dtype)
    if mutant != "flow_no_row_mask":
        h = torch.where(mask[:, :, None], h, torch.zeros((), dtype=dtype))
    return flow_finish_ref(h @ W.to(dtype).T + bias.to(dtype), flow, x0, mask, dtype, mutant)


def flow_euler_ref(x_t, velocity, dt, mask, dtype=F64):
    """out = x_t + velocity * dt (product, then sum), times the [B, L] row mask when given."""
    out = x_t.to(dtype) + velocity.to(dtype) * _r32(dt)
    return out if mask is None else out * mask.to(dtype)[:, :, None]


# (B, L): 16 rows per workgroup, 4 per wave; the finalizer sums 1024 utterances per trip
FLOW_HEAD_CASES = [(1, 1), (2, 3), (3, 16), (2, 17), (5, 37), (1030, 2)]
FLOW_HEAD_WIDE = (2, 17)        # y is the column slice [:, :, 4:260] of a [B, L, 264] tensor
FLOW_HEAD_NAN = (5, 37)         # the masked rows of y hold NaN
# (B, L, C): 16 lanes per utterance, 64 utterances per pass, ratios kept in LDS for B <= 1024
FLOW_FINISH_CASES = [(1, 1, 1), (3, 5, 1), (2, 6, 3), (5, 37, 3), (70, 37, 3), (1100, 2, 3)]
FLOW_EULER_CASES = [(1, 1, 1), (5, 37, 3), (3, 100, 3)]
FLOW_EULER_DT = [0.125, 0.1]
FLOW_SIGMA = 1e-5


def flow_lens(B, L):
    return [b % (L + 1) for b in range(B)] if B > 64 else _lens(B, L)


def flow_finish_inputs(case):
    B, L, C = case
    seed = 3000 + 10 * FLOW_FINISH_CASES.index(case)
    return dict(raw=rand(case, seed), flow=rand(case, seed + 1), x0=rand(case, seed + 2), mask=_len_mask(flow_lens(B, L), L))


def flow_mix_inputs(case):
    B, L, C = case
    seed = 3200 + 10 * FLOW_FINISH_CASES.index(case)
    t = torch.rand((B,), generator=torch.Generator().manual_seed(seed + 2))
    t[0] = 1.0
    if B > 1:
        t[1] = 0.0
    return dict(x0=rand(case, seed), x1=rand(case, seed + 1, 2.0) + 0.3, t=t, sigma=FLOW_SIGMA)


def flow_head_inputs(case):
    """-> dict(y, wide, gamma, beta, eps, W, bias, flow, x0, mask); y is a view of `wide` where that is not None."""
    B, L = case
    seed = 3400 + 10 * FLOW_HEAD_CASES.index(case)
    mask = _len_mask(flow_lens(B, L), L)
    y = rand((B, L, 256), seed, 2.0) + 0.3
    if case == FLOW_HEAD_NAN:
        y[~mask] = float("nan")
    wide = None
    if case == FLOW_HEAD_WIDE:
        wide = rand((B, L, 264), seed + 7)
        wide[:, :, 4:260] = y
        y = wide[:, :, 4:260]
    return dict(y=y, wide=wide, gamma=1.0 + 0.1 * rand((256,), seed + 1), beta=rand((256,), seed + 2, 0.1), eps=1e-5,
                W=rand((3, 256), seed + 3, 256 ** -0.5), bias=rand((3,), seed + 4, 0.1), flow=rand((B, L, 3), seed + 5),
                x0=rand((B, L, 3), seed + 6), mask=mask)


def flow_euler_inputs(case, masked):
    B, L, C = case
    seed = 3600 + 10 * FLOW_EULER_CASES.index(case)
    return dict(x_t=rand(case, seed), velocity=rand(case, seed + 1, 3.0), mask=_len_mask(_lens(B, L) if B > 1 else [0], L) if masked else None)


# ------------------------------------------------------------------------------------------------ infer_features


def infer_features_ref(pred, duration_target, pitch_target, energy_target, duration_factor=1.0, pitch_factor=1.0, pitch_delta=0.0,
                       energy_factor=1.0, energy_delta=0.0, round_duration=False, dtype=F64, mutant=None):
    """duration = max(df (exp(pred[..., 0]) - 1), 0) (rounded half to even before the clamp with `round_duration`), replaced by the
    target wherever that is >= 0; features = { (pitch_target | pred[..., 1]) pf + pd, (energy_target | pred[..., 2]) ef + ed }.
    The factors are the float arguments of the C entry point.  -> duration [B, L], features [B, L, 2]."""
    p = pred.to(dtype)
    d = _r32(duration_factor) * (torch.exp(p[..., 0]) - 1.0)
    if round_duration:
        d = torch.round(d)
    d = torch.clamp(d, min=0.0)
    if duration_target is not None:
        t = duration_target.to(dtype)
        d = torch.where(t > 0 if mutant == "infer_target_gt_0" else t >= 0, t, d)
    pitch = p[..., 1] if pitch_target is None else pitch_target.to(dtype)
    energy = p[..., 2] if energy_target is None else energy_target.to(dtype)
    return d, torch.stack([pitch * _r32(pitch_factor) + _r32(pitch_delta), energy * _r32(energy_factor) + _r32(energy_delta)], dim=-1)


INFER_CASES = [(1, 1), (3, 37), (2, 300)]
INFER_TARGETS = ["none", "dur_f32", "dur_i64", "pitch", "energy", "pitch_energy"]
INFER_FACTORS = {"default": {}, "scaled": dict(duration_factor=1.3, pitch_factor=0.9, pitch_delta=0.25, energy_factor=1.1, energy_delta=-0.5)}


def infer_inputs(case, targets):
    """pred [B, L, 3]; the duration targets hold zeros (token 1 among them, whose predicted duration is e - 1: `> 0` instead of
    `>= 0` shows there) and negative entries (about a third of the fp32 target, -1 in the int64 one)."""
    B, L = case
    seed = 4000 + 10 * INFER_CASES.index(case)
    pred = rand((B, L, 3), seed)
    g = torch.Generator().manual_seed(seed + 1)
    dur = torch.randint(0, 8, (B, L), generator=g)
    neg = torch.rand((B, L), generator=g) < 1.0 / 3.0
    if L > 1:
        pred[0, 1, 0], dur[0, 1], neg[0, 1], neg[0, 0] = 1.0, 0, False, True
    duration_target = None
    if targets == "dur_f32":
        duration_target = torch.where(neg, -1.0 - torch.rand((B, L), generator=g), dur.float())
    elif targets == "dur_i64":
        duration_target = torch.where(neg, torch.full_like(dur, -1), dur)
    return dict(pred=pred, duration_target=duration_target, pitch_target=rand((B, L), seed + 2) if "pitch" in targets else None,
                energy_target=rand((B, L), seed + 3) if "energy" in targets else None)


# ------------------------------------------------------------------------------------------------ time embedding, token embedding


def time_embedding_ref(t, inv_freq, freq_scale, w0, b0, w1, b1, dtype=F64):
    """out = W1 silu(W0 f + b0) + b1 over f = [t, sin a, cos a], the argument a rounded as the kernel rounds it (time_features)."""
    n = t.numel()
    if n == 0:
        return torch.zeros((0, w1.shape[0]), dtype=dtype)
    return time_embedding_fwd(time_features(t, inv_freq, freq_scale, dtype), w0.to(dtype), b0.to(dtype), w1.to(dtype), b1.to(dtype))


# (n, H, E): one wave per time value, lane j < E owns hidden unit j and output j; H, E <= 64
TIME_FWD_SHAPES = [(1, 32, 32), (67, 32, 32), (5, 1, 1), (3, 64, 64), (4, 7, 33), (0, 32, 32)]


def time_fwd_inputs(n, H, E):
    """time_inputs of train_kernels_reference (t in [0, 1] with exact 0 and 1, arguments up to 1000 rad) plus b1; n = 0: no t."""
    i = time_inputs(max(n, 1), H, E)
    i.pop("d_out")
    if n == 0:
        i["t"] = i["t"][:0]
    i["b1"] = rand((E,), 116, 0.1)
    return i


def embed_tokens_ref(text, table, text_len, dtype=F64, mutant=None):
    """emb[b][l] = table[text[b][l]], ids outside [0, V) read row 0; mask[b][l] = l < text_len[b] (None: all ones)."""
    V = table.shape[0]
    bad = (text < 0) | (text >= V)
    ids = torch.where(bad, torch.full_like(text, V - 1 if mutant == "embed_clamp_last" else 0), text)
    B, L = text.shape
    mask = torch.ones((B, L), dtype=torch.bool) if text_len is None else _len_mask(text_len, L)
    return table.to(dtype)[ids], mask


# (V, D, B, L): one wave per token row, 4 rows per workgroup, D / 4 float4 over 64 lanes
EMBED_CASES = [(149, 384, 5, 77), (3, 4, 1, 1), (10, 260, 3, 2)]
EMBED_WIDE = (10, 260, 3, 2)        # the table is the slice [:, 4:4 + D] of a [V, D + 8] tensor
EMBED_BAD_IDS = (-1, None, 2 ** 40)  # None = V


def embed_inputs(case):
    """-> dict(text, table, wide, text_len, bad): ids in range with -1, V and 2^40 planted at `bad` (flat positions) when there are
    at least three ids; the table's row 0 is not zero.  `table` is a view of `wide` where that is not None."""
    V, D, B, L = case
    seed = 5000 + 10 * EMBED_CASES.index(case)
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(1, V, (B, L), generator=g)
    bad = []
    if B * L >= 3:
        bad = [1, (B * L) // 2, B * L - 1]
        for pos, v in zip(bad, EMBED_BAD_IDS):
            text.view(-1)[pos] = V if v is None else v
    table, wide = rand((V, D), seed + 1), None
    if case == EMBED_WIDE:
        wide = rand((V, D + 8), seed + 2)
        wide[:, 4:4 + D] = table
        table = wide[:, 4:4 + D]
    return dict(text=text, table=table, wide=wide, text_len=torch.tensor(_lens(B, L)), bad=bad)


OTHER_MUTANTS = ["infer_target_gt_0", "embed_clamp_last"]

# ------------------------------------------------------------------------------------------------ fp32 noise
# max over the case tables of rel_err(fp32 evaluation on the CPU, float64 reference), per kernel output: measured by
# tests/test_adaptor_reference_host.py::test_fp32_noise_table (which prints the per-case figures and fails when an entry here
# is below what it measures, or more than a factor 4 above).  torch's sums and the BLAS behind `@` choose their order by CPU and
# thread count, so the figures differ between machines (up to a factor 2.2 between the two kinds this was measured on): each
# entry is the larger of the two measurements.  A kernel is allowed 8 x its figure, and never more than 1e-4.
FP32_NOISE = {
    "length_regulate.out": 2.755e-7,
    "soft_average.log_duration": 2.718e-8, "soft_average.targets": 5.845e-7,
    "flow_head.pred": 3.369e-7, "flow_head.duration": 6.043e-7, "flow_head.ratio": 2.955e-7, "flow_head.loss": 1.697e-7,
    "flow_finish.duration": 2.198e-7, "flow_finish.ratio": 9.089e-8, "flow_finish.loss": 5.613e-8,
    "infer_features.duration": 2.841e-7,
    "time_embedding.out": 2.849e-7,
}


def tol(key: str) -> float:
    return min(8.0 * FP32_NOISE[key], TOL_CAP)


def measure_fp32_noise() -> dict:
    """key -> {case label: rel_err of the fp32 evaluation} over every case of the kernels whose tolerance is measured."""
    out: dict = {k: {} for k in FP32_NOISE}

    def put(kernel, names, label, lo, hi):
        for name, a, b in zip(names, lo, hi):
            out[f"{kernel}.{name}"][label] = rel_err(a, b)

    for case in LR_CASES:
        i = lr_inputs(case, "align_i64", exact=False)
        args = (i["x"], i["dur"], i["alignment"], i["M"], i["max_len"], None)
        put("length_regulate", ("out",), f"{case}", length_regulate_ref(*args, dtype=F32), length_regulate_ref(*args))
    for case in SA_CASES:
        i = sa_inputs(case)
        args = (i["attn"], i["pitch"], i["energy"], i["duration"], i["text_len"])
        lo, hi = soft_average_ref(*args, dtype=F32), soft_average_ref(*args)
        put("soft_average", ("log_duration", "targets"), f"{case}", (lo[..., 0], lo[..., 1:]), (hi[..., 0], hi[..., 1:]))
    for case in FLOW_HEAD_CASES:
        i = flow_head_inputs(case)
        i.pop("wide")
        put("flow_head", ("pred", "duration", "ratio", "loss"), f"{case}", flow_head_ref(**i, dtype=F32), flow_head_ref(**i))
    for case in FLOW_FINISH_CASES:
        i = flow_finish_inputs(case)
        lo, hi = flow_finish_ref(**i, dtype=F32), flow_finish_ref(**i)
        put("flow_finish", ("duration", "ratio", "loss"), f"{case}", lo[1:], hi[1:])
    for case in INFER_CASES:
        i = infer_inputs(case, "none")
        for fname, fac in INFER_FACTORS.items():
            for rnd in (False, True):
                put("infer_features", ("duration",), f"{case} {fname}{' round' if rnd else ''}",
                    infer_features_ref(**i, **fac, round_duration=rnd, dtype=F32), infer_features_ref(**i, **fac, round_duration=rnd))
    for shape in TIME_FWD_SHAPES:
        i = time_fwd_inputs(*shape)
        put("time_embedding", ("out",), f"{shape}", (time_embedding_ref(**i, dtype=F32),), (time_embedding_ref(**i),))
    return out
