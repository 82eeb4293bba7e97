"""The float64 references of tests/adaptor_reference.py against the project's oracle and plain PyTorch expressions (agreement
to float64 rounding, or exact where the inputs make the arithmetic exact), the fp32-noise figures from which
tests/test_gpu_adaptor_kernels.py takes its measured tolerances, and the mutants: deliberately wrong references that the case
tables must tell from the true ones.  CPU only.

Which cases kill which mutant (KILLS below; every pair is asserted)
  lr_drop_last_chunk       L % 16 != 0: (1, 63, 15, 256) and (3, 65, 17, 384) with an alignment, (2, 130, 33, 384) on the soft path
  lr_no_enc_len_mask       soft path with enc_len: (1, 63, 15, 256) enc_len 9, (2, 64, 16, 256) enc_len 0, (3, 65, 17, 384) enc_len 16
  lr_no_max_len_clamp      max_len below the sum: (1, 63, 15, 256), (2, 64, 16, 256), (2, 128, 48, 384) - dec_len and dec_mask, and
                           on the soft path the rows between max_len and the sum
  lr_no_dec_len_mask       soft path, max_len below the sum and below M: (1, 63, 15, 256), (2, 128, 48, 384)
  lr_swap_tile_halves      M > 32: (1, 63, 15, 256) a partial tile, (2, 64, 16, 256) a full one, (2, 130, 33, 384) the third tile
  lr_second_feature_group  every case: (2, 1, 1, 256) NT = 2, (3, 65, 17, 384) NT = 3
  sa_no_tail               (2, 112, 64) every frame, (2, 113, 63), (2, 129, 64) frame 128 alone, (1, 300, 130)
  sa_no_tail_after         (2, 129, 64), (1, 300, 130)
  sa_no_text_len           (2, 15, 5), (3, 17, 65): utterances with text_len 0 and below L
  flow_first_1024          flow_head (1030, 2), flow_finish (1100, 2, 3): the loss
  flow_no_floor            flow_head (2, 3), flow_finish (3, 5, 1): an utterance without a valid row divides 0 by 0
  flow_no_row_mask         flow_head (5, 37): the masked rows of y hold NaN
  infer_target_gt_0        (3, 37) and (2, 300) with an fp32 and an int64 target: token (0, 1) has target 0
  embed_clamp_last         (149, 384, 5, 77), (10, 260, 3, 2): ids -1, V and 2^40
"""
import pytest
import torch
import torch.nn.functional as F

import adaptor_reference as R
from isp_tts_amd.utils import masked_mean
from oracle import acoustic_oracle as orc

TOL = 1e-12
F32 = torch.float32


def _exact_in_16_bits(t):
    return torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t)


# ------------------------------------------------------------------------------------------------ references


@pytest.mark.parametrize("mode", R.LR_MODES)
@pytest.mark.parametrize("case", R.LR_CASES)
def test_length_regulate_ref(case, mode):
    """With an alignment: bmm.  Without: the oracle's generate_soft_path + bmm, evaluated in fp32 - the exact inputs make the fp32
    and the float64 evaluations the same numbers.  dec_len = (dur.sum(1) + 0.5).long(), clamped."""
    B, M, L, D = case
    i = R.lr_inputs(case, mode)
    x, dur, A, max_len, enc_len = i["x"], i["dur"], i["alignment"], i["max_len"], i["enc_len"]
    out, dl, mask = R.length_regulate_ref(x, dur, A, M, max_len, enc_len)
    out32, dl32, _ = R.length_regulate_ref(x, dur, A, M, max_len, enc_len, dtype=F32)
    want_dl = (dur.sum(1) + 0.5).long()
    if max_len >= 0:
        want_dl = want_dl.clamp(max=max_len)
    assert dl.dtype == torch.int64 and torch.equal(dl, want_dl) and torch.equal(dl32, want_dl)
    assert torch.equal(mask, torch.arange(M)[None] < want_dl[:, None])
    assert out.dtype == torch.float64 and out32.dtype == F32 and torch.equal(out32.double(), out), "the exact inputs are not exact"
    assert _exact_in_16_bits(x) and float(x.abs().max()) <= 64
    if A is not None:
        assert _exact_in_16_bits(A) and float(A.abs().max()) <= 4
        assert torch.equal(out, torch.bmm(A.double(), x.double()))
    else:
        assert dur.dtype == F32 and torch.equal(dur * 4, (dur * 4).round()) and 0 <= float(dur.min()) and float(dur.max()) <= 6
        el = torch.full((B,), L) if enc_len is None else enc_len
        m3 = (torch.arange(L)[None] < el[:, None]).unsqueeze(2) & (torch.arange(M)[None] < want_dl[:, None]).unsqueeze(1)
        path = orc.generate_soft_path(dur, m3.float()).transpose(1, 2)
        assert path.dtype == F32 and torch.equal(out32, torch.bmm(path, x.contiguous()))
        for b in range(B):
            if int(dl[b]) == 0 or int(el[b]) == 0:
                assert float(out[b].abs().max()) == 0.0
            assert float(out[b, int(dl[b]):].abs().max() if int(dl[b]) < M else 0.0) == 0.0


def test_length_regulate_inputs_hold_the_conditions():
    """max_len = -1 with a sum above M; max_len below the sum (and below M); an utterance of zero durations; enc_len with 0 and L
    when B > 1; non-zero durations behind enc_len; a row-strided x on both paths."""
    seen = set()
    for case in R.LR_CASES:
        B, M, L, D = case
        for mode in ("align_i64", "soft_enc"):
            i = R.lr_inputs(case, mode)
            raw, dl = R.dec_len_ref(i["dur"]), R.dec_len_ref(i["dur"], i["max_len"])
            if i["max_len"] < 0 and bool((raw > M).any()):
                seen.add((mode, "unclamped above M"))
            if i["max_len"] >= 0 and bool((raw > i["max_len"]).any()):
                seen.add((mode, "clamped"))
                if i["max_len"] < M:
                    seen.add((mode, "clamped below M"))
            if bool((i["dur"].sum(1) == 0).any()):
                assert 0 in dl.tolist()
                seen.add((mode, "all zero"))
            if i["wide"] is not None:
                assert i["x"].stride(1) == D + 16 and i["x"].data_ptr() == i["wide"].data_ptr() + 32
                seen.add((mode, "strided x"))
            if mode == "soft_enc":
                el = i["enc_len"]
                if B > 1:
                    assert 0 in el.tolist() and L in el.tolist()
                behind = i["dur"] * (torch.arange(L)[None] >= el[:, None])
                if bool(((behind.sum(1) > 0) & (el > 0)).any()):
                    seen.add((mode, "durations behind enc_len"))
                if bool(((behind.sum(1) > 0) & (el == 0)).any()):
                    seen.add((mode, "durations behind enc_len 0"))
    want = {(m, c) for m in ("align_i64", "soft_enc") for c in ("unclamped above M", "clamped", "clamped below M", "all zero", "strided x")}
    want |= {("soft_enc", "durations behind enc_len"), ("soft_enc", "durations behind enc_len 0")}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("case", R.SA_CASES)
def test_soft_average_ref(case):
    B, M, L = case
    i = R.sa_inputs(case)
    attn, tl = i["attn"], i["text_len"]
    mk = (torch.arange(L)[None] < tl[:, None]).double()
    got = R.soft_average_ref(attn, i["pitch"], i["energy"], i["duration"], tl)
    for col, dense in ((1, i["pitch"]), (2, i["energy"])):
        want = orc.soft_average(dense[:, None].double(), attn.double()).transpose(1, 2)[..., 0] * mk
        R.close(got[..., col], want, TOL, f"column {col}")
    assert torch.equal(got[..., 0], torch.log1p(i["duration"].double())) and 0 in i["duration"].tolist()[0]
    assert float(R.soft_average_ref(attn, i["pitch"], i["energy"], None, tl)[..., 0].abs().max()) == 0.0
    if i["zero_col"] is not None:
        assert float(attn[:, :, i["zero_col"]].abs().max()) == 0.0 and float(got[:, i["zero_col"], 1:].abs().max()) == 0.0
    if B > 1:
        assert 0 in tl.tolist() and L in tl.tolist()
    assert float((got[..., 1:] * (1 - mk)[..., None]).abs().max()) == 0.0


@pytest.mark.parametrize("case", R.FLOW_FINISH_CASES)
def test_flow_mix_and_finish_ref(case):
    """The expressions of FlowTransformerTemporalModule.forward as tests/test_gpu_kernels.py restates them, and utils.masked_mean."""
    B, L, C = case
    m = R.flow_mix_inputs(case)
    x0, x1, sigma, tt = m["x0"], m["x1"], m["sigma"], m["t"][:, None, None]
    xt, flow = R.flow_mix_ref(**m, dtype=F32)
    assert torch.equal(xt, (1 - (1 - sigma) * tt) * x0 + tt * x1) and torch.equal(flow, x1 - (1 - sigma) * x0)
    xt64, flow64 = R.flow_mix_ref(**m)
    R.close(xt64, (1 - (1 - sigma) * tt.double()) * x0.double() + tt.double() * x1.double(), TOL, "x_t")
    R.close(xt, xt64, 1e-6, "x_t fp32") and R.close(flow, flow64, 1e-6, "flow fp32")
    i = R.flow_finish_inputs(case)
    raw, fl, x0, mask = i["raw"].double(), i["flow"].double(), i["x0"].double(), i["mask"]
    m3 = mask[..., None].expand(-1, -1, C)
    pf = raw * m3
    pred, dur, ratio, loss = R.flow_finish_ref(**i)
    assert torch.equal(pred, (x0 + pf) * m3)
    assert torch.equal(dur, torch.clamp(torch.exp(pred[..., 0]) - 1, min=0))
    R.close(loss, masked_mean(F.mse_loss(pf, fl, reduction="none"), m3), TOL, "loss")
    R.close(ratio.mean(), loss, TOL, "mean of the ratios")
    assert ratio.shape == (B,) and loss.shape == () and bool(torch.isfinite(ratio).all())
    lens = mask.sum(1)
    assert (0 in lens.tolist()) == (B > 1) and float(ratio[lens == 0].abs().max() if B > 1 else 0.0) == 0.0
    assert float(pred[~mask].abs().max() if B > 1 else 0.0) == 0.0 and float(dur[~mask].abs().max() if B > 1 else 0.0) == 0.0
    # pred in fp32 is one rounding per operation: the expression in fp32
    p32 = R.flow_finish_ref(**i, dtype=F32)[0]
    assert torch.equal(p32, (i["x0"] + i["raw"] * m3) * m3)


@pytest.mark.parametrize("case", R.FLOW_HEAD_CASES)
def test_flow_head_ref(case):
    B, L = case
    i = R.flow_head_inputs(case)
    wide = i.pop("wide")
    y, mask = i["y"], i["mask"]
    if case == R.FLOW_HEAD_WIDE:
        assert y.stride(1) == 264 and y.data_ptr() == wide.data_ptr() + 16
    clean = torch.where(mask[..., None], y, torch.zeros(())).double()
    if case == R.FLOW_HEAD_NAN:
        assert bool(torch.isnan(y[~mask]).all()) and bool((~mask).any()) and bool(torch.isfinite(y[mask]).all())
    h = F.layer_norm(clean, (256,), i["gamma"].double(), i["beta"].double(), float(torch.tensor(1e-5, dtype=F32))) * mask[..., None]
    raw = F.linear(h, i["W"].double(), i["bias"].double())
    want = R.flow_finish_ref(raw, i["flow"], i["x0"], mask)
    got = R.flow_head_ref(**i)
    for name, g, w in zip(("pred", "duration", "ratio", "loss"), got, want):
        assert bool(torch.isfinite(g).all()), name
        R.close(g, w, TOL, name)
    lens = mask.sum(1).tolist()
    assert L in lens and ((0 in lens) == (B > 1))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", R.FLOW_EULER_CASES)
def test_flow_euler_ref(case, masked):
    i = R.flow_euler_inputs(case, masked)
    for dt in R.FLOW_EULER_DT:
        want = i["x_t"] + i["velocity"] * dt
        if masked:
            want = want * i["mask"][..., None]
            assert 0 in i["mask"].sum(1).tolist()
        assert torch.equal(R.flow_euler_ref(i["x_t"], i["velocity"], dt, i["mask"], dtype=F32), want)
        R.close(R.flow_euler_ref(i["x_t"], i["velocity"], dt, i["mask"]), want, 1e-6, "float64 against fp32")


@pytest.mark.parametrize("rnd", [False, True])
@pytest.mark.parametrize("fname", list(R.INFER_FACTORS))
@pytest.mark.parametrize("targets", R.INFER_TARGETS)
@pytest.mark.parametrize("case", R.INFER_CASES)
def test_infer_features_ref(case, targets, fname, rnd):
    """FlowTemporalAdaptor.infer between predictor and embedding stack, with torch.round / clamp / where."""
    B, L = case
    i, fac = R.infer_inputs(case, targets), R.INFER_FACTORS[fname]
    f = dict(duration_factor=1.0, pitch_factor=1.0, pitch_delta=0.0, energy_factor=1.0, energy_delta=0.0)
    f.update({k: float(torch.tensor(v, dtype=F32)) for k, v in fac.items()})
    p = i["pred"].double()
    d = f["duration_factor"] * (torch.exp(p[..., 0]) - 1)
    if rnd:      # no value within 16 fp32 ulps of a tie, where another exp could round it the other way
        assert bool((((d - torch.floor(d)) - 0.5).abs() > 16 * 2.0 ** -23 * d.abs().clamp(min=1.0)).all())
        d = torch.round(d)
    d = torch.clamp(d, min=0)
    t = i["duration_target"]
    if t is not None:
        t = t.double()
        d = torch.where(t < 0, d, t)
        assert L == 1 or (bool((t < 0).any()) and float(t[0, 1]) == 0.0 and float(i["pred"][0, 1, 0]) == 1.0)
        if targets == "dur_f32" and L > 1:
            assert 0.2 < float((t < 0).double().mean()) < 0.45
        if targets == "dur_i64" and L > 1:
            assert i["duration_target"].dtype == torch.int64 and float(t.min()) == -1.0
    pitch = p[..., 1] if i["pitch_target"] is None else i["pitch_target"].double()
    energy = p[..., 2] if i["energy_target"] is None else i["energy_target"].double()
    want_f = torch.stack([pitch * f["pitch_factor"] + f["pitch_delta"], energy * f["energy_factor"] + f["energy_delta"]], -1)
    got_d, got_f = R.infer_features_ref(**i, **fac, round_duration=rnd)
    R.close(got_d, d, TOL, "duration")
    R.close(got_f, want_f, TOL, "features")
    # in fp32 the features are one rounding per operation
    p32 = i["pred"]
    pitch = p32[..., 1] if i["pitch_target"] is None else i["pitch_target"]
    energy = p32[..., 2] if i["energy_target"] is None else i["energy_target"]
    want32 = torch.stack([pitch * fac.get("pitch_factor", 1.0) + fac.get("pitch_delta", 0.0),
                          energy * fac.get("energy_factor", 1.0) + fac.get("energy_delta", 0.0)], -1)
    assert torch.equal(R.infer_features_ref(**i, **fac, round_duration=rnd, dtype=F32)[1], want32)


@pytest.mark.parametrize("n,H,E", R.TIME_FWD_SHAPES)
def test_time_embedding_ref(n, H, E):
    i = R.time_fwd_inputs(n, H, E)
    got = R.time_embedding_ref(**i)
    assert got.shape == (n, E) and got.dtype == torch.float64
    if n == 0:
        return
    if n > 1:
        assert float(i["t"].min()) == 0.0 and float(i["t"].max()) == 1.0
    f = R.time_features(i["t"], i["inv_freq"], i["freq_scale"])
    want = F.linear(F.silu(F.linear(f, i["w0"].double(), i["b0"].double())), i["w1"].double(), i["b1"].double())
    R.close(got, want, TOL, "out")


def test_time_embedding_ref_against_the_oracle(state_dict):
    """At the model's shape: the oracle forms the argument in the same order, so the two agree to fp32 evaluation noise."""
    p = "temporal_adaptor.predictor.time_embedding"
    t = R.time_fwd_inputs(67, 32, 32)["t"]
    inv_freq = 1000.0 ** -(torch.arange(32).float() / 32)
    got = R.time_embedding_ref(t, inv_freq, state_dict[f"{p}.freq_emb.freq_scale"], state_dict[f"{p}.mlp.0.weight"],
                               state_dict[f"{p}.mlp.0.bias"], state_dict[f"{p}.mlp.2.weight"], state_dict[f"{p}.mlp.2.bias"])
    R.close(orc.time_embedding(state_dict, t), got, 1e-5, "oracle")


@pytest.mark.parametrize("case", R.EMBED_CASES)
def test_embed_tokens_ref(case):
    V, D, B, L = case
    i = R.embed_inputs(case)
    text, table = i["text"], i["table"]
    if case == R.EMBED_WIDE:
        assert table.stride(0) == D + 8 and table.data_ptr() == i["wide"].data_ptr() + 16
    emb, mask = R.embed_tokens_ref(text, table, i["text_len"], dtype=F32)
    flat = text.reshape(-1)
    good = torch.ones(B * L, dtype=torch.bool)
    good[i["bad"]] = False
    assert bool(((flat[good] >= 0) & (flat[good] < V)).all())
    assert torch.equal(emb.reshape(-1, D)[good], F.embedding(flat[good], table))
    if i["bad"]:
        assert flat[i["bad"]].tolist() == [-1, V, 2 ** 40]
        assert torch.equal(emb.reshape(-1, D)[i["bad"]], table[0].expand(3, D)) and float(table[0].abs().min()) > 0.0
    assert torch.equal(mask, torch.arange(L)[None] < i["text_len"][:, None]) and (B == 1 or 0 in i["text_len"].tolist())
    assert bool(R.embed_tokens_ref(text, table, None)[1].all())


# ------------------------------------------------------------------------------------------------ fp32 noise


def test_fp32_noise_table():
    """Measures what an fp32 evaluation of each formula loses against float64 at every case, prints it, and fails when a recorded
    figure of adaptor_reference.FP32_NOISE (max over the cases, rounded up) is below the measurement - or more than a factor 4
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


# ------------------------------------------------------------------------------------------------ mutants

KILLS = {
    "lr_drop_last_chunk": [((1, 63, 15, 256), "align_i64"), ((3, 65, 17, 384), "align_f32"), ((2, 130, 33, 384), "soft")],
    "lr_no_enc_len_mask": [((1, 63, 15, 256), "soft_enc"), ((2, 64, 16, 256), "soft_enc"), ((3, 65, 17, 384), "soft_enc")],
    "lr_no_max_len_clamp": [((1, 63, 15, 256), "align_i64"), ((2, 64, 16, 256), "align_i64_sum"), ((2, 128, 48, 384), "soft")],
    "lr_no_dec_len_mask": [((1, 63, 15, 256), "soft"), ((2, 128, 48, 384), "soft_enc")],
    "lr_swap_tile_halves": [((1, 63, 15, 256), "align_i64"), ((2, 64, 16, 256), "soft"), ((2, 130, 33, 384), "align_i64")],
    "lr_second_feature_group": [((2, 1, 1, 256), "align_i64"), ((3, 65, 17, 384), "soft")],
    "sa_no_tail": [(2, 112, 64), (2, 113, 63), (2, 129, 64), (1, 300, 130)],
    "sa_no_tail_after": [(2, 129, 64), (1, 300, 130)],
    "sa_no_text_len": [(2, 15, 5), (3, 17, 65)],
    "flow_first_1024": [("head", (1030, 2)), ("finish", (1100, 2, 3))],
    "flow_no_floor": [("head", (2, 3)), ("finish", (3, 5, 1))],
    "flow_no_row_mask": [("head", (5, 37))],
    "infer_target_gt_0": [((3, 37), "dur_f32"), ((2, 300), "dur_i64")],
    "embed_clamp_last": [(149, 384, 5, 77), (10, 260, 3, 2)],
}


def test_every_mutant_is_listed():
    assert set(KILLS) == set(R.LR_MUTANTS + R.SA_MUTANTS + R.FLOW_MUTANTS + R.OTHER_MUTANTS)


@pytest.mark.parametrize("name,case,mode", [(n, c, m) for n in R.LR_MUTANTS for c, m in KILLS[n]])
def test_length_regulate_mutants_are_killed(name, case, mode):
    """These checks are exact: any difference in out, dec_len or dec_mask kills."""
    i = R.lr_inputs(case, mode)
    args = (i["x"], i["dur"], i["alignment"], i["M"], i["max_len"], i["enc_len"])
    true, wrong = R.length_regulate_ref(*args), R.length_regulate_mutant(name, *args)
    assert any(R.differs(w, t) for w, t in zip(wrong, true))
    if name in ("lr_swap_tile_halves", "lr_second_feature_group", "lr_drop_last_chunk", "lr_no_enc_len_mask", "lr_no_dec_len_mask"):
        assert R.differs(wrong[0], true[0])         # these leave the lengths alone: the rows must show them


@pytest.mark.parametrize("name,case", [(n, c) for n in R.SA_MUTANTS for c in KILLS[n]])
def test_soft_average_mutants_are_killed(name, case):
    i = R.sa_inputs(case)
    args = (i["attn"], i["pitch"], i["energy"], i["duration"], i["text_len"])
    assert R.differs(R.soft_average_ref(*args, mutant=name)[..., 1:], R.soft_average_ref(*args)[..., 1:], R.tol("soft_average.targets"))


@pytest.mark.parametrize("name,which,case", [(n, w, c) for n in R.FLOW_MUTANTS for w, c in KILLS[n]])
def test_flow_mutants_are_killed(name, which, case):
    if which == "head":
        i = R.flow_head_inputs(case)
        i.pop("wide")
        true, wrong = R.flow_head_ref(**i), R.flow_head_ref(**i, mutant=name)
    else:
        i = R.flow_finish_inputs(case)
        true, wrong = R.flow_finish_ref(**i), R.flow_finish_ref(**i, mutant=name)
    keys = [f"flow_{which}.{k}" for k in ("pred", "duration", "ratio", "loss")]
    tols = [None if k == "flow_finish.pred" else R.tol(k) for k in keys]
    killed = [k for k, w, t, tl in zip(keys, wrong, true, tols) if R.differs(w, t, tl)]
    assert killed, name
    if name == "flow_first_1024":
        assert killed == [f"flow_{which}.loss"]


@pytest.mark.parametrize("case,targets", KILLS["infer_target_gt_0"])
def test_infer_features_mutant_is_killed(case, targets):
    i = R.infer_inputs(case, targets)
    for rnd in (False, True):
        true = R.infer_features_ref(**i, round_duration=rnd)[0]
        assert R.differs(R.infer_features_ref(**i, round_duration=rnd, mutant="infer_target_gt_0")[0], true, R.tol("infer_features.duration"))


@pytest.mark.parametrize("case", KILLS["embed_clamp_last"])
def test_embed_tokens_mutant_is_killed(case):
    i = R.embed_inputs(case)
    assert R.differs(R.embed_tokens_ref(i["text"], i["table"], i["text_len"], mutant="embed_clamp_last")[0],
                     R.embed_tokens_ref(i["text"], i["table"], i["text_len"])[0])
