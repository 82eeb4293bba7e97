"""The float64 references of tests/aligner_reference.py against the project's oracle (forwards) and float64 autograd over the
forward references (backwards), the fp32-noise figures from which tests/test_gpu_aligner_kernels.py takes its measured
tolerances, the derived bound of the fast scores path, the condition on the prior's cutoff, and the mutants: deliberately wrong
references that the case tables must tell from the true ones at the tolerance the GPU test uses.  CPU only.

Which cases kill which mutant (KILLS below; every pair is asserted)
  scores_block_swapped               every L above 32: (2, 33, 33) NB 2, (2, 65, 65) 3, (2, 130, 100) 4, (2, 33, 129) and (2, 65, 160) 5,
                                     (2, 31, 161) 6, (2, 32, 193) 7, (2, 64, 226) 8, (2, 1, 257) 9, (2, 130, 289) and (3, 65, 320) 10
  scores_lse_over_text_len           text_len below L: (2, 1, 31), (2, 130, 100), (3, 65, 320)
  scores_prior_unclamped_len         lengths 0 or above the size: (2, 31, 1), (3, 32, 32), (2, 64, 64), (2, 65, 160)
  scores_row_32_dropped              M > 32: (2, 33, 33) wave 1's only row, (2, 65, 65), (2, 130, 100) rows 32 and 96
  instnorm_no_tail / _var            every n > 1: (3, 17, 65), (3, 112, 63) the tail is everything, (2, 113, 160), (3, 129, 64) frame 128
                                     alone, (3, 300, 80)
  instnorm_var_unbiased              (3, 17, 65), (3, 300, 80)
  instnorm_bwd_no_c2                 (1, 17, 65), (3, 33, 64), (1, 300, 1)
  instnorm_bwd_param_last_utterance  B > 1: (3, 33, 64), (2, 9, 260)
  scores_bwd_sg_over_L               d_soft given, text_len below L: (2, 2, 64) soft, (1, 5, 65) both, (3, 33, 65) soft
  scores_bwd_no_logsoftmax_term      (1, 5, 65) logits, (5, 1, 130) both, (1, 5, 320) both (d_soft alone leaves sum_j dA = 0: the term vanishes)
  sa_bwd_no_eps                      an all-zero column inside text_len: (1, 63, 4), (2, 130, 7)
  sa_bwd_mask_ignored                text_len below L: (1, 63, 4), (1, 65, 5) text_len 0, (5, 130, 1)
  pad_split_no_clamp                 every case (1e6 is planted in each): (1, 1, 1), (2, 29, 33)
"""
import pytest
import torch
import torch.nn.functional as F

import aligner_reference as R
from oracle import acoustic_oracle as orc

TOL = 1e-10     # float64 against float64 (the ill-conditioned instance-norm channel costs five digits)
F32, F64 = torch.float32, torch.float64


def _clamped(lengths, lo, hi):
    return torch.as_tensor(lengths).clamp(lo, hi)


# ------------------------------------------------------------------------------------------------ pad_rows


@pytest.mark.parametrize("case", list(R.PAD_CASES))
def test_pad_rows_ref(case):
    B, T, C = case
    i = R.pad_inputs(case)
    v, channel_first, x = R.pad_view(i["base"], case)
    lens = i["lengths"]
    layout = R.PAD_CASES[case]
    if layout == "cf":
        assert channel_first and v.shape == (B, C, T) and v.stride(2) == 1 and v.stride(1) == T + 3 > 1
    if layout == "cl_wide":
        assert v.stride(1) == C + 16 and v.data_ptr() == i["base"].data_ptr() + 32
    n = _clamped(lens, 0, T)
    want = torch.zeros(B, T + 4, C)
    if B <= 64:
        for b in range(B):
            want[b, 2:2 + int(n[b])] = x[b, :int(n[b])]
    else:
        want[:, 2:T + 2] = x * (torch.arange(T)[None] < n[:, None])[..., None] + 0.0        # (+ 0.0: no negative zeros)
    got = R.pad_rows_ref(x, lens, dtype=F32)
    assert torch.equal(got, want) and torch.equal(R.pad_rows_ref(x, lens).float(), want)
    assert torch.equal(R.pad_rows_ref(x, lens, "bf16"), want.to(torch.bfloat16))
    planes = R.pad_rows_ref(x, lens, "split")
    clamped = want.clamp(-65504.0, 65504.0)
    assert planes.shape == (2, B, T + 4, C) and planes.dtype == torch.float16 and torch.equal(planes[0], clamped.half())
    assert bool(torch.isfinite(planes).all())
    assert bool(((planes[0].double() + planes[1].double() - clamped.double()).abs() <= R.split_bound(want)).all())
    assert int(n[0]) == T and float(x[0, 0, 0]) == 1e6 and float(want.abs().max()) == 1e6
    if T * C >= 4:
        assert sorted(x[0].reshape(-1)[:4].tolist()) == sorted(torch.tensor(R.PAD_SPECIALS).tolist())


def test_pad_rows_lengths_hold_the_conditions():
    """0, 1, T and T + 3 (clamped) under both kernels; the fallback case holds all of them."""
    for layout in ("cl", "cf"):
        seen = set()
        for case, lay in R.PAD_CASES.items():
            B, T, C = case
            if lay.startswith(layout) and B <= 64:
                seen |= {("T+3" if v == T + 3 else "T" if v == T else v) for v in R.pad_lengths(case).tolist()}
        assert {0, 1, "T", "T+3"} <= seen, (layout, seen)
    assert set(R.pad_lengths((65536, 1, 2)).tolist()) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------ masked instance norm


@pytest.mark.parametrize("case", list(R.INSTNORM_CASES))
def test_masked_instnorm_ref_against_the_oracle(case):
    B, T, C = case
    i = R.instnorm_inputs(case)
    y, lens = i["y"], i["lengths"]
    n = _clamped(lens, 1, T)                                  # the oracle's domain: 1 <= len <= T
    got = R.masked_instnorm_ref(**i)
    assert got.dtype == F64 and got.shape == (B, T + 4, C) and bool(torch.isfinite(got).all())
    x = torch.nan_to_num(y[:, :T], nan=0.0).double().transpose(1, 2)            # [B, C, T]
    mask = (torch.arange(T)[None] < n[:, None])[:, None, :]
    want = orc.masked_instance_norm(x, mask, i["weight"].double(), i["bias"].double(), float(torch.tensor(1e-5, dtype=F32)))
    want = want.transpose(1, 2)
    for b in range(B):
        nb = int(n[b])
        assert bool(torch.isnan(y[b, nb:]).all()) and bool(torch.isfinite(y[b, :nb]).all())
        R.close(got[b, 2:2 + nb], want[b, :nb], TOL, f"utterance {b}")
        assert float(got[b, :2].abs().max()) == 0.0 and float(got[b, 2 + nb:].abs().max()) == 0.0
        if nb == 1:
            assert torch.equal(got[b, 2], i["bias"].double())
        if C >= 3:
            assert torch.equal(got[b, 2:2 + nb, R.INSTNORM_CONST_CHANNEL], i["bias"][R.INSTNORM_CONST_CHANNEL].double().expand(nb))
            ill = y[b, :nb, R.INSTNORM_ILL_CHANNEL].double()
            assert float(ill.mean()) == 1000.0 and (nb < 2 or 1e-2 <= float(ill.std(unbiased=False)) <= 3.2e-2)
            # every partial sum of the channel is exact in fp32: the fp32 evaluation has the mean exactly
            assert float(y[b, :nb, R.INSTNORM_ILL_CHANNEL].sum()) == 1000.0 * nb
            if nb >= 2:     # ... and an uncentred variance is lost entirely
                v32 = y[b, :nb, R.INSTNORM_ILL_CHANNEL]
                one_pass = float((v32 * v32).mean() - v32.mean() ** 2)
                assert abs(one_pass - float(ill.var(unbiased=False))) > 0.5 * float(ill.var(unbiased=False))


def test_instnorm_lengths_hold_the_conditions():
    fwd = {(n, n == T) for (B, T, C), lens in R.INSTNORM_CASES.items() for n in _clamped(lens, 1, T).tolist()}
    assert {(n, whole) for n in (1, 15, 16, 17, 112, 113, 129, 300) for whole in (True, False)} <= fwd
    assert {C for (B, T, C) in R.INSTNORM_CASES} >= {1, 63, 64, 65, 80, 160}
    assert R.INSTNORM_CASES[(3, 17, 65)] == (17, 1, 9)
    bwd = {n for (B, T, C), lens in R.INSTNORM_BWD_CASES.items() for n in _clamped(lens, 1, T).tolist()}
    assert {1, 15, 16, 17, 33, 300} <= bwd and {B for (B, T, C) in R.INSTNORM_BWD_CASES} >= {1, 3} and (2, 9, 260) in R.INSTNORM_BWD_CASES
    raw = [v for lens in list(R.INSTNORM_CASES.values()) + list(R.INSTNORM_BWD_CASES.values()) for v in lens]
    assert 0 in raw and 20 in raw


@pytest.mark.parametrize("case", list(R.INSTNORM_BWD_CASES))
def test_masked_instnorm_bwd_ref_against_autograd(case):
    B, T, C = case
    i = R.instnorm_inputs(case, backward=True)
    n = _clamped(i["lengths"], 1, T)
    y = i["y"].double().requires_grad_(True)
    w, bias = i["weight"].double().requires_grad_(True), i["bias"].double().requires_grad_(True)
    out = R.masked_instnorm_ref(y, w, bias, i["lengths"])
    loss = sum((out[b, 2:2 + int(n[b])] * i["d_out"][b, :int(n[b])].double()).sum() for b in range(B))
    gy, gw, gb = torch.autograd.grad(loss, (y, w, bias))
    d_y, dw, db = R.masked_instnorm_bwd_ref(i["y"], i["d_out"], i["weight"], i["lengths"])
    assert bool(torch.isfinite(d_y).all()) and bool(torch.isfinite(gy).all())
    R.close(d_y, gy, TOL, "d_y")
    R.close(dw, gw, TOL, "d_weight")
    R.close(db, gb, TOL, "d_bias")
    for b in range(B):
        assert float(d_y[b, int(n[b]):].abs().max()) == 0.0 and bool(torch.isnan(i["d_out"][b, int(n[b]):]).all())


# ------------------------------------------------------------------------------------------------ scores


def _oracle_scores(q, k, tl, ml):
    """oracle.conv_attention from the matmul on (its lines after the projections), in float64: q [B, M, D], k [B, L, D]."""
    kmask = orc.get_mask_from_lengths(tl).unsqueeze(1)
    qmask = orc.get_mask_from_lengths(ml).unsqueeze(1)
    mask = qmask.transpose(1, 2) & kmask
    attn = torch.matmul(q, k.transpose(1, 2)) * R.SCALE
    attn = torch.clamp(attn, max=orc.F32_MAX)
    prior = orc.batch_diagonal_prior(tl.double(), ml.double())
    attn = F.log_softmax(attn, dim=2) + torch.log(prior + 1e-6)
    logits = attn.clone()
    attn = attn.masked_fill(~mask[:, :1], orc.F32_MIN)
    return F.softmax(attn, dim=2) * mask, logits


@pytest.mark.parametrize("case", list(R.SCORES_CASES))
def test_aligner_scores_ref_against_the_oracle(case):
    B, M, L = case
    i = R.scores_inputs(case)
    q, k = i["q"], i["k"]
    assert bool(torch.isnan(q[:, M:]).all()) and bool(torch.isnan(k[:, L:]).all())
    assert bool(torch.isfinite(q[:, :M]).all()) and bool(torch.isfinite(k[:, :L]).all())
    if case == R.SCORES_Q_SLICE:
        assert q.stride(0) == 2 * (M + 4) * R.AD and q.data_ptr() == i["wide"].data_ptr()
    tl, ml = _clamped(i["text_len"], 1, L), _clamped(i["mel_len"], 1, M)      # the oracle's domain
    assert int(tl.max()) == L and int(ml.max()) == M
    soft, logits = R.aligner_scores_ref(q, k, i["text_len"], i["mel_len"], M, L)
    want_soft, want_logits = _oracle_scores(q[:, :M].double(), k[:, :L].double(), tl, ml)
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(soft).all())
    R.close(logits, want_logits, 1e-12, "logits")
    R.close(soft, want_soft, 1e-12, "soft")
    dead_keys = torch.arange(L)[None, None, :] >= tl[:, None, None]
    dead_rows = torch.arange(M)[None, :, None] >= ml[:, None, None]
    assert float((soft * (dead_keys | dead_rows)).abs().max()) == 0.0
    R.close(soft.sum(-1)[R.live_rows(case)], torch.ones(int(R.live_rows(case).sum()), dtype=F64), 1e-12, "row sums")
    if case == R.SCORES_BIG:
        s = q[:, :M].double() @ k[:, :L].double().transpose(1, 2) * R.SCALE
        assert 79.9 < float(s.abs().max()) < 80.1


def test_scores_cases_hold_the_conditions():
    Ls = [L for (B, M, L) in R.SCORES_CASES]
    assert Ls == [1, 31, 32, 33, 64, 65, 100, 129, 160, 161, 193, 226, 257, 289, 320]
    assert {(L + 31) // 32 for L in Ls} == set(range(1, 11))
    assert {M for (B, M, L) in R.SCORES_CASES} == {1, 31, 32, 33, 64, 65, 130}
    tls = {("L" if v == L else "L+5" if v == L + 5 else "in" if 1 < v < L and v % 32 else v)
           for (B, M, L), (tl, ml) in R.SCORES_CASES.items() for v in tl}
    mls = {("M" if v == M else "M+7" if v == M + 7 else v) for (B, M, L), (tl, ml) in R.SCORES_CASES.items() for v in ml}
    assert {"L", 1, 0, "L+5", "in"} <= tls and {"M", 1, 0, "M+7"} <= mls
    for (B, M, L), (tl, ml) in R.SCORES_CASES.items():
        assert M == 1 or any(max(v, 1) < M for v in ml), "one utterance has mel_len < M"
    bm = {B * M for (B, M, L) in R.SCORES_BWD_CASES}
    assert {1, 4, 5} <= bm and {L for (B, M, L) in R.SCORES_BWD_CASES} >= {1, 63, 64, 65, 130, 320}
    assert any(L % 4 and M % 4 for (B, M, L) in R.SCORES_BWD_CASES)
    raw = [(v, L) for (B, M, L), (tl, ml) in R.SCORES_BWD_CASES.items() for v in tl]
    raw += [(v, M) for (B, M, L), (tl, ml) in R.SCORES_BWD_CASES.items() for v in ml]
    assert any(v == 0 for v, s in raw) and any(v > s for v, s in raw)


@pytest.mark.parametrize("mode", R.SCORES_BWD_MODES)
@pytest.mark.parametrize("case", list(R.SCORES_BWD_CASES))
def test_aligner_scores_bwd_ref_against_autograd(case, mode):
    """Autograd from the unscaled product q.k on (the kernel's dS is the gradient of that product), with the NaN of d_soft's
    unread columns replaced by 0 for autograd alone."""
    B, M, L = case
    i = R.scores_bwd_inputs(case, mode)
    P = (i["q"][:, :M].double() @ i["k"][:, :L].double().transpose(1, 2)).requires_grad_(True)
    soft, logits = R.aligner_scores_ref(i["q"], i["k"], i["text_len"], i["mel_len"], M, L, product=P)
    loss = 0.0
    if i["d_soft"] is not None:
        tl = _clamped(i["text_len"], 1, L)
        assert bool(torch.isnan(i["d_soft"]).any()) == bool((tl < L).any())
        loss = loss + (soft * torch.nan_to_num(i["d_soft"], nan=0.0).double()).sum()
    if i["d_logits"] is not None:
        loss = loss + (logits * i["d_logits"].double()).sum()
    want, = torch.autograd.grad(loss, P)
    got = R.aligner_scores_bwd_ref(logits.detach(), soft.detach(), i["d_soft"], i["d_logits"], i["text_len"], i["mel_len"])
    assert bool(torch.isfinite(got).all())
    R.close(got, want, TOL, "dS")
    if mode == "soft":
        dead = ~R.live_rows(case, R.SCORES_BWD_CASES)
        assert float(got[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0
    assert i["logits"].dtype == F32 and torch.equal(i["logits"], logits.detach().float()) and torch.equal(i["soft"], soft.detach().float())


# ------------------------------------------------------------------------------------------------ soft averages, backward


@pytest.mark.parametrize("case", list(R.SA_BWD_CASES))
def test_soft_average_bwd_ref_against_autograd(case):
    B, M, L = case
    i = R.sa_bwd_inputs(case)
    A = i["attn"].double().requires_grad_(True)
    feats = R.soft_average_ref(A, i["pitch"], i["energy"], None, i["text_len"])
    want, = torch.autograd.grad((feats * i["d_feats"].double()).sum(), A)
    got = R.soft_average_bwd_ref(i["attn"], i["pitch"], i["energy"], i["d_feats"], i["text_len"])
    R.close(got, want, TOL, "dA")
    masked = torch.arange(L)[None] >= i["text_len"][:, None]
    assert float((got * masked[:, None, :]).abs().max()) == 0.0
    if i["zero_col"] is not None:
        assert float(i["attn"][:, :, i["zero_col"]].abs().max()) == 0.0
    acc = R.soft_average_bwd_ref(i["attn"], i["pitch"], i["energy"], i["d_feats"], i["text_len"], prior=i["prior"])
    assert torch.equal(acc, i["prior"].double() + got)


def test_soft_average_bwd_cases_hold_the_conditions():
    assert {B * L for (B, M, L) in R.SA_BWD_CASES} >= {1, 4, 5} and {M for (B, M, L) in R.SA_BWD_CASES} >= {1, 63, 64, 65, 130}
    sizes = {B * M * L for (B, M, L) in R.SA_BWD_CASES}
    assert 256 in sizes and 257 in sizes and any(s < 256 for s in sizes)
    tls = [(v, L) for (B, M, L), tl in R.SA_BWD_CASES.items() for v in tl]
    assert any(v == 0 for v, L in tls) and any(v == L for v, L in tls)
    assert any(tl[b] > 1 and L > 1 for (B, M, L), tl in R.SA_BWD_CASES.items() for b in range(B)), "a zero column inside text_len"


# ------------------------------------------------------------------------------------------------ fp32 noise


def test_fp32_noise_table():
    """Measures what an fp32 evaluation of each formula loses against float64 at every case, prints it, and fails when a recorded
    figure of aligner_reference.FP32_NOISE (max over the cases, rounded up) is below the measurement - or more than a factor 4
    above it (the order of torch's sums, and so the figure, depends on the CPU: see adaptor_reference.FP32_NOISE)."""
    measured = R.measure_fp32_noise()
    print("\nfp32 evaluation on the CPU against float64, max |diff| / max |ref|")
    for key, per_case in measured.items():
        worst = max(per_case.values())
        print(f"  {key:28s} measured {worst:.3e}  recorded {R.FP32_NOISE[key]:.3e}  -> tolerance {R.tol(key):.3e}")
        for label, e in per_case.items():
            print(f"      {label:60s} {e:.3e}")
    for key, per_case in measured.items():
        worst = max(per_case.values())
        assert worst <= R.FP32_NOISE[key] <= worst * 4, f"{key}: recorded {R.FP32_NOISE[key]:.3e}, measured {worst:.3e}"
        assert R.tol(key) <= R.TOL_CAP


# ------------------------------------------------------------------------------------------------ the prior's cutoff


def test_prior_cutoff_band():
    """The band is at least 16 x the distance of the fp32 prior from float64 (measured and printed), and what it leaves out is
    little: at most 2 % of a case's live rows, at most one row of a case with fewer than 50, and never a whole 32-row wave tile."""
    d = R.measure_prior_fp32_distance()
    print(f"\nfp32 prior against float64, max relative distance over the cells >= 1e-5: {d:.3e} (recorded {R.PRIOR_FP32_DISTANCE:.3e}); "
          f"band {R.PRIOR_BAND:.1e} = {R.PRIOR_BAND / d:.1f} x")
    assert d <= R.PRIOR_FP32_DISTANCE <= 4 * d and R.PRIOR_BAND >= 16 * R.PRIOR_FP32_DISTANCE
    for table in (R.SCORES_CASES, R.SCORES_BWD_CASES):
        for case in table:
            B, M, L = case
            _, rows = R.scores_checked(case, table)
            live = R.live_rows(case, table)
            out = int((~rows & live).sum())
            print(f"  {case}: {out} of {int(live.sum())} live rows have a borderline cell")
            assert out <= 0.02 * int(live.sum()) or (int(live.sum()) < 50 and out <= 1), case
            if int(live.sum()) < 50:
                assert out <= 1, case
            assert not bool((~rows & ~live).any())
            for b in range(B):
                for m0 in range(0, M, 32):
                    assert bool(rows[b, m0:m0 + 32].any()), (case, b, m0)


# ------------------------------------------------------------------------------------------------ the fast path's bound


@pytest.mark.parametrize("case", list(R.SCORES_CASES))
def test_fast_path_bound(case):
    """The float64 emulation of the three-term bf16 product stays inside the derived bound (its product term alone, without the
    fp32 tolerance and the transcendental term); an emulation without either cross term leaves the whole bound by at least 16 x
    wherever L >= 32."""
    B, M, L = case
    i = R.scores_inputs(case)
    q, k = i["q"], i["k"]
    args = (q, k, i["text_len"], i["mel_len"], M, L)
    soft, logits = R.aligner_scores_ref(*args)
    cells, rows = R.scores_checked(case)
    product_only = R.fast_logit_bound(q, k, M, L, 0.0) - R.fast_transcendental_term(q, k, M, L)
    full = R.fast_logit_bound(q, k, M, L, R.tol("scores.logits") * float(logits.abs().max()))
    s3, l3 = R.aligner_scores_ref(*args, product=R.split_bf16_product(q[:, :M], k[:, :L]))
    worst = float(((l3 - logits).abs() / product_only).max())
    print(f"{case}: three-term emulation, worst |diff| / product term = {worst:.3f}; "
          f"transcendental term {R.fast_transcendental_term(q, k, M, L):.3e}")
    assert worst <= 1.0
    soft_bound = R.tol("scores.soft") + 2 * full.max(-1, keepdim=True).values
    assert bool(((s3 - soft).abs() <= soft_bound).all())
    if L >= 32:
        for drop in ("q_lo", "k_lo"):
            _, l2 = R.aligner_scores_ref(*args, product=R.split_bf16_product(q[:, :M], k[:, :L], drop=drop))
            ratio = float(((l2 - logits).abs() / full)[cells].max())
            print(f"    without the {drop} cross term: worst |diff| / bound = {ratio:.1f}")
            assert ratio >= 16.0, (drop, ratio)


# ------------------------------------------------------------------------------------------------ mutants

KILLS = {
    "scores_block_swapped": [c for c in R.SCORES_CASES if c[2] > 32],
    "scores_lse_over_text_len": [(2, 1, 31), (2, 130, 100), (3, 65, 320)],
    "scores_prior_unclamped_len": [(2, 31, 1), (3, 32, 32), (2, 64, 64), (2, 65, 160)],
    "scores_row_32_dropped": [(2, 33, 33), (2, 65, 65), (2, 130, 100)],
    "instnorm_no_tail": [(3, 17, 65), (3, 112, 63), (2, 113, 160), (3, 129, 64), (3, 300, 80)],
    "instnorm_no_tail_var": [(3, 17, 65), (3, 112, 63), (2, 113, 160), (3, 129, 64), (3, 300, 80)],
    "instnorm_var_unbiased": [(3, 17, 65), (3, 300, 80)],
    "instnorm_bwd_no_c2": [(1, 17, 65), (3, 33, 64), (1, 300, 1)],
    "instnorm_bwd_param_last_utterance": [(3, 33, 64), (2, 9, 260)],
    "scores_bwd_sg_over_L": [((2, 2, 64), "soft"), ((1, 5, 65), "both"), ((3, 33, 65), "soft")],
    "scores_bwd_no_logsoftmax_term": [((1, 5, 65), "logits"), ((5, 1, 130), "both"), ((1, 5, 320), "both")],
    "sa_bwd_no_eps": [(1, 63, 4), (2, 130, 7)],
    "sa_bwd_mask_ignored": [(1, 63, 4), (1, 65, 5), (5, 130, 1)],
    "pad_split_no_clamp": [(1, 1, 1), (2, 29, 33)],
}


def test_every_mutant_is_listed():
    assert set(KILLS) == set(R.SCORES_MUTANTS + R.INSTNORM_MUTANTS + R.INSTNORM_BWD_MUTANTS + R.SCORES_BWD_MUTANTS + R.SA_BWD_MUTANTS
                             + R.PAD_MUTANTS)
    assert {(L + 31) // 32 for (B, M, L) in KILLS["scores_block_swapped"]} == set(range(2, 11))


@pytest.mark.parametrize("name,case", [(n, c) for n in R.SCORES_MUTANTS for c in KILLS[n]])
def test_scores_mutants_are_killed(name, case):
    """On the cells and rows the GPU test compares, at its tolerances."""
    B, M, L = case
    i = R.scores_inputs(case)
    args = (i["q"], i["k"], i["text_len"], i["mel_len"], M, L)
    (soft, logits), (wsoft, wlogits) = R.aligner_scores_ref(*args), R.aligner_scores_ref(*args, mutant=name)
    cells, rows = R.scores_checked(case)
    by_logits = R.differs(wlogits[cells], logits[cells], R.tol("scores.logits"))
    by_soft = R.differs(wsoft[rows], soft[rows], R.tol("scores.soft"))
    assert by_logits or by_soft
    if name in ("scores_block_swapped", "scores_lse_over_text_len"):
        assert by_logits


@pytest.mark.parametrize("name,case", [(n, c) for n in R.INSTNORM_MUTANTS for c in KILLS[n]])
def test_instnorm_mutants_are_killed(name, case):
    i = R.instnorm_inputs(case)
    assert R.differs(R.masked_instnorm_ref(**i, mutant=name), R.masked_instnorm_ref(**i), R.tol("instnorm.out"))


@pytest.mark.parametrize("name,case", [(n, c) for n in R.INSTNORM_BWD_MUTANTS for c in KILLS[n]])
def test_instnorm_bwd_mutants_are_killed(name, case):
    i = R.instnorm_inputs(case, backward=True)
    i.pop("bias")
    true, wrong = R.masked_instnorm_bwd_ref(**i), R.masked_instnorm_bwd_ref(**i, mutant=name)
    which = 1 if name == "instnorm_bwd_param_last_utterance" else 0
    assert R.differs(wrong[which], true[which], R.tol("instnorm_bwd.d_weight" if which else "instnorm_bwd.d_y"))


@pytest.mark.parametrize("name,case,mode", [(n, c, m) for n in R.SCORES_BWD_MUTANTS for c, m in KILLS[n]])
def test_scores_bwd_mutants_are_killed(name, case, mode):
    i = R.scores_bwd_inputs(case, mode)
    args = (i["logits"], i["soft"], i["d_soft"], i["d_logits"], i["text_len"], i["mel_len"])
    _, rows = R.scores_checked(case, R.SCORES_BWD_CASES)
    assert R.differs(R.aligner_scores_bwd_ref(*args, mutant=name)[rows], R.aligner_scores_bwd_ref(*args)[rows], R.tol("scores_bwd.dS"))


@pytest.mark.parametrize("name,case", [(n, c) for n in R.SA_BWD_MUTANTS for c in KILLS[n]])
def test_soft_average_bwd_mutants_are_killed(name, case):
    i = R.sa_bwd_inputs(case)
    args = (i["attn"], i["pitch"], i["energy"], i["d_feats"], i["text_len"])
    assert R.differs(R.soft_average_bwd_ref(*args, mutant=name), R.soft_average_bwd_ref(*args), R.tol("soft_average_bwd.dA"))


@pytest.mark.parametrize("case", KILLS["pad_split_no_clamp"])
def test_pad_rows_mutant_is_killed(case):
    i = R.pad_inputs(case)
    x = R.pad_view(i["base"], case)[2]
    assert R.differs(R.pad_rows_ref(x, i["lengths"], "split", mutant="pad_split_no_clamp")[0], R.pad_rows_ref(x, i["lengths"], "split")[0])
