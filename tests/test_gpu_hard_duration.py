"""GPU: hard durations (FlowTemporalAdaptor with soft_duration off, the reference's constructor default).

The three kernels of csrc/hard_duration.hip against CPU restatements (tests/hard_duration_reference.py) at the smallest shapes
where each can go wrong, the rounded `infer` durations, and the model - forward, `infer`, the training step, graph capture -
against outputs of the reference itself (tests/golden/hard_duration.npz, tools/make_hard_duration_goldens.py)."""
import numpy as np
import pytest
import torch

from conftest import crc, golden

import hard_duration_reference as hdr
from isp_tts_amd import graph, runtime, synth, train
from isp_tts_amd.acoustic import AcousticModel
from isp_tts_amd.config import AcousticDims

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEL_TOL = 1e-4                  # the project's fp32 bar
INFER_BF16_MEL_TOL = 2e-1       # the bound tests/test_gpu_model.py states for `infer` on the bf16 path (with 3e-2 relative RMS)
U = 2.0 ** -24                  # unit roundoff of fp32


def _maxdiff(a, b) -> float:
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a)
    return float((a.double() - torch.as_tensor(b).double()).abs().max())


def _sparse_durations(B, L, seed):
    """Mostly zeros: about one token in thirty has frames, the first and the last token among them."""
    g = torch.Generator().manual_seed(seed)
    dur = torch.randint(1, 21, (B, L), generator=g) * (torch.rand(B, L, generator=g) < 1 / 30)
    dur[:, 0], dur[:, -1] = 2, 3
    dur[0, L // 2] = 500                                   # one long run; utterance 0 overflows 600 frames, utterance 1 does not
    return dur.long()


def _ragged_durations(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    dur = torch.randint(0, 5, (B, L), generator=g)
    dur[1] = torch.randint(0, 3, (L,), generator=g)        # utterance 0 sums to about 2 L (more than 130 frames), utterance 1 to L
    return dur.long()


REGULATOR_CASES = {   # name -> (durations [B, L], frames, max_len)
    "minimal": (torch.tensor([[1]]), 1, None),
    "zero_runs": (torch.tensor([[0, 3, 0, 4, 0], [12, 0, 0, 0, 0], [1, 1, 1, 1, 1]]), 12, None),
    "cut_inside_a_token": (torch.tensor([[0, 3, 0, 4, 0], [12, 0, 0, 0, 0], [1, 1, 1, 1, 1]]), 12, 6),
    "scan_across_waves": (_ragged_durations(2, 70, 1), 130, None),
    "token_limit": (_sparse_durations(2, 512, 2), 600, None),
    "fractional": (torch.tensor([[0.49, 0.5, 1.5, 2.4999, 3.0]]), 8, None),
}


def _strided_rows(B, L, D, seed):
    """x [B, L, D] as a view of wider rows (ldx = D + 8 > D)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, D + 8, generator=g)[..., :D]


@pytest.mark.parametrize("D", [256, 384])
@pytest.mark.parametrize("case", list(REGULATOR_CASES))
def test_hard_regulate_is_the_row_gather(case, D):
    """ispk_hard_regulate_f32: bit-equal to x[b, token of frame y] built on the CPU, zero rows behind the last token, decoder
    lengths and mask from the same launch; x a strided view."""
    dur, frames, max_len = REGULATOR_CASES[case]
    B, L = dur.shape
    x = _strided_rows(B, L, D, 3)
    want, want_len = hdr.hard_regulate(x, dur, max_len=max_len, frames=frames)
    xd = x.to(DEV)
    xd = torch.empty(B, L, D + 8, device=DEV)[..., :D].copy_(xd)
    assert xd.stride(1) == D + 8
    out, dec_len, mask = runtime.hard_regulate(xd, dur.to(DEV), frames, max_len=-1 if max_len is None else max_len)
    torch.cuda.synchronize()
    assert torch.equal(dec_len.cpu(), want_len)
    assert torch.equal(mask.cpu(), torch.arange(frames)[None] < want_len[:, None])
    assert torch.equal(out.cpu(), want)
    if case == "fractional":
        assert want_len.tolist() == [8] and torch.equal(hdr.repeats(dur), torch.tensor([[0, 1, 2, 2, 3]]))
    if case == "cut_inside_a_token":
        assert want_len.tolist() == [6, 6, 5] and not out[:, 6:].any()
    if case == "token_limit":
        assert int(want_len[0]) > frames > int(want_len[1])            # one utterance fills every row, one leaves a zero tail


@pytest.mark.parametrize("D", [256, 384])
@pytest.mark.parametrize("case", list(REGULATOR_CASES))
def test_hard_regulate_backward_sums_each_tokens_rows(case, D):
    """ispk_hard_regulate_bwd_f32 against float64 segment sums: within n 2^-24 max|d_out| for a token of n frames (first-order
    bound of an fp32 sum of n terms), exactly zero for tokens without frames, the same bits on a second run."""
    dur, frames, max_len = REGULATOR_CASES[case]
    B, L = dur.shape
    g = torch.Generator().manual_seed(5)
    d_out = torch.randn(B, frames, D, generator=g)
    reps = hdr.repeats(dur)
    ends = torch.cumsum(reps, 1)
    total = ends[:, -1] if max_len is None else ends[:, -1].clamp(max=max_len)
    valid = total.clamp(max=frames)
    want = torch.zeros(B, L, D, dtype=torch.float64)
    n = torch.zeros(B, L)
    for b in range(B):
        for l in range(L):
            lo, hi = min(int(ends[b, l] - reps[b, l]), int(valid[b])), min(int(ends[b, l]), int(valid[b]))
            want[b, l] = d_out[b, lo:hi].double().sum(0)
            n[b, l] = hi - lo
    args = (d_out.to(DEV), dur.to(DEV), -1 if max_len is None else max_len)
    got = runtime.hard_regulate_bwd(*args)
    again = runtime.hard_regulate_bwd(*args)
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    got = got.cpu()
    err = (got.double() - want).abs().amax(dim=2)
    bound = n * U * float(d_out.abs().max())
    print(f"{case} D={D}: worst error / bound = {float((err / bound.clamp(min=1e-30)).max()):.3f}, longest token {int(n.max())} frames")
    assert bool((err <= bound).all())
    assert not got[n == 0].any() and bool((n == 0).any()) == (case != "minimal")


AVERAGER_CASES = {   # name -> (durations [B, L], text_len, M)
    "small": (torch.tensor([[5, 0, 7, 3, 0, 20, 5], [0, 0, 6, 30, 4, 0, 0], [10, 10, 10, 10, 0, 0, 0]]), torch.tensor([7, 5, 3]), 40),
    "one_long_token": (torch.tensor([[10, 1700, 13]]), torch.tensor([3]), 1723),
}


@pytest.mark.parametrize("case", list(AVERAGER_CASES))
def test_hard_average_is_the_mean_of_the_nonzero_frames(case):
    """ispk_hard_average_f32 against float64 direct means: tokens without frames, an all-zero (unvoiced) segment, partly zero
    segments, text_len below L (masked tokens give 0), a token of 1,700 frames; the log1p column within 2 ulp."""
    dur, text_len, M = AVERAGER_CASES[case]
    B, L = dur.shape
    g = torch.Generator().manual_seed(7)
    pitch = torch.randn(B, M, generator=g) + 3.0
    energy = torch.rand(B, M, generator=g) * 4.0
    pitch[:, 3::7] = 0.0                                   # partly zero segments
    if case == "small":
        pitch[0, 12:15] = 0.0                              # token 3 of utterance 0: unvoiced
        energy[1, 0:6] = 0.0                               # token 2 of utterance 1
    mask = torch.arange(L)[None] < text_len[:, None]
    want = torch.stack([torch.log1p(dur.double()), hdr.hard_average(pitch, dur) * mask, hdr.hard_average(energy, dur) * mask], dim=-1)
    got = runtime.hard_average(pitch.to(DEV), energy.to(DEV), dur.to(DEV), text_len.to(DEV)).cpu()
    n = dur.clamp(min=0).double()
    for c, x in ((1, pitch), (2, energy)):
        err = (got[..., c].double() - want[..., c]).abs()
        bound = n * U * float(x.abs().max())
        print(f"{case} column {c}: worst error / bound = {float((err / bound.clamp(min=1e-30)).max()):.3f}")
        assert bool((err <= bound).all())
    ulp = torch.from_numpy(np.spacing(want[..., 0].float().numpy()))
    assert bool(((got[..., 0].double() - want[..., 0]).abs() <= 2 * ulp.double()).all())
    if case == "small":
        assert got[0, 3, 1] == 0 and got[1, 2, 2] == 0 and want[0, 3, 2] != 0            # unvoiced segments give exactly 0
        assert not got[1, 5:, 1:].any() and not got[2, 3:, 1:].any() and want[2, 2, 1] != 0   # masked tokens; the last valid one
        assert float(got[0, 0, 1]) != float(pitch[0, :5].mean())                         # zeros are left out of the mean


def test_infer_features_round_half_to_even():
    """ispk_infer_features_round_f32: durations rounded like torch.round before the clamp, targets >= 0 in their place unrounded;
    the features as ispk_infer_features_f32 computes them."""
    pre = torch.tensor([0.5, 1.5, 2.5, 3.49, 3.51, -0.4, -0.6, -3.0, 0.0, 7.0, 2.5000002, 1e-3])
    pred = torch.zeros(1, pre.numel(), 3)
    pred[0, :, 0] = torch.log1p(pre.clamp(min=-0.99))
    pred[0, :, 1:] = torch.randn(pre.numel(), 2, generator=torch.Generator().manual_seed(1))
    raw = torch.exp(pred[..., 0]) - 1
    d = pred.to(DEV)
    dur, feats = runtime.infer_features(d, None, None, None, round_duration=True)
    soft, feats_soft = runtime.infer_features(d, None, None, None)
    # the kernel's expf may differ from torch's in the last bit: round what the KERNEL computed (its unrounded sibling's output)
    assert torch.equal(dur.cpu(), torch.clamp(torch.round(soft.cpu()), min=0)) and torch.equal(feats, feats_soft)
    far = (raw - (torch.floor(raw) + 0.5)).abs() > 1e-3
    assert torch.equal(dur.cpu()[far], torch.clamp(torch.round(raw), min=0)[far])
    assert torch.equal(torch.round(torch.tensor([0.5, 1.5, 2.5])), torch.tensor([0.0, 2.0, 2.0]))
    target = torch.full((1, pre.numel()), -1.0)
    target[0, ::2] = 2.25
    dur_t, _ = runtime.infer_features(d, target.to(DEV), None, None, round_duration=True)
    assert torch.equal(dur_t.cpu(), torch.where(target < 0, dur.cpu(), target))
    dur2, _ = runtime.infer_features(d, None, None, None, duration_factor=2.0, round_duration=True)
    soft2, _ = runtime.infer_features(d, None, None, None, duration_factor=2.0)
    assert torch.equal(dur2, torch.clamp(torch.round(soft2), min=0))


def test_modules_take_the_hard_branch_without_an_alignment():
    """LengthRegulator.forward(x, durations, max_len) and TemporalAverager.forward(x, durations) with the reference's signatures."""
    from isp_tts_amd.acoustic.temporal_adaptor import LengthRegulator, TemporalAverager
    dur = REGULATOR_CASES["zero_runs"][0]
    x = _strided_rows(3, 5, 256, 4).contiguous()
    reg = LengthRegulator()
    out, dec = reg(x.to(DEV), dur.to(DEV), max_len=9)               # the output length is read back: longest utterance, cut to 9
    want, want_len = hdr.hard_regulate(x, dur, max_len=9)
    assert out.shape == (3, 9, 256) and torch.equal(out.cpu(), want) and torch.equal(dec.cpu(), want_len)
    assert torch.equal(reg.dec_mask.cpu(), torch.arange(9)[None] < want_len[:, None])
    out, dec = reg(x.to(DEV), dur.float().to(DEV))
    assert out.shape == (3, 12, 256) and torch.equal(out.cpu(), hdr.hard_regulate(x, dur)[0])
    dense = torch.randn(3, 3, 12, generator=torch.Generator().manual_seed(2))
    dense[:, :, 5] = 0.0
    avg = TemporalAverager()(dense.to(DEV), dur.to(DEV)).cpu()
    assert avg.shape == (3, 3, 5)
    for c in range(3):
        assert _maxdiff(avg[:, c], hdr.hard_average(dense[:, c], dur)) <= 12 * U * float(dense.abs().max())


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def hard_model(state_dict):
    """The product model with hard durations on the GPU, frozen (the inference kernels), with the synthetic weights - the same
    state_dict the soft-duration model loads."""
    runtime.lib()
    model = AcousticModel.init(AcousticDims().model_config(soft_duration=False)).eval()
    model.load_state_dict(state_dict, strict=True)
    return model.to(DEV).requires_grad_(False)


@pytest.fixture(scope="module")
def fixture_and_inputs():
    g = golden("hard_duration.npz")
    inp = hdr.fixture_inputs()
    assert [crc(inp[k]) for k in ("text", "mel", "pitch", "energy")] == [int(v) for v in g["inputs_crc"]]
    return g, {k: v.to(DEV) for k, v in inp.items()}


def test_forward_against_the_reference_fixture(hard_model, fixture_and_inputs):
    g, inp = fixture_and_inputs
    out = hard_model(**inp)
    torch.cuda.synchronize()
    ao = out.adaptor_output
    assert np.array_equal(out.aligner_output.attn_hard_duration.cpu().numpy(), g["duration_target"])
    assert np.array_equal(ao.dec_lengths.cpu().numpy(), g["dec_lengths"])
    assert torch.equal(ao.dec_mask.cpu(), torch.arange(512)[None] < torch.from_numpy(g["dec_lengths"])[:, None])
    longest = int(g["duration_target"].max())
    d = {"pitch_target": _maxdiff(ao.pitch_target, g["pitch_target"]), "energy_target": _maxdiff(ao.energy_target, g["energy_target"]),
         "mel": _maxdiff(out.mel[:, :, ::int(g["mel_row_step"])], g["mel_rows"]),
         "log_duration": _maxdiff(ao.log_duration, g["log_duration"]),
         "flow_loss": abs(float(ao.losses["flow_loss"]) - float(g["flow_loss"]))}
    print("hard-duration forward vs reference: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items())
          + f" (d_avg {g['d_avg'][0]:.2e} / {g['d_avg'][1]:.2e}, d_mel {float(g['d_mel']):.2e}, longest token {longest} frames)")
    # the reference's own averager noise (d_avg) plus the kernel's bound for the longest token
    assert d["pitch_target"] <= g["d_avg"][0] + longest * U * float(inp["pitch"].abs().max())
    assert d["energy_target"] <= g["d_avg"][1] + longest * U * float(inp["energy"].abs().max())
    assert out.mel.shape == (2, 80, 512) and d["mel"] <= MEL_TOL + float(g["d_mel"])
    assert d["log_duration"] < 1e-4 and d["flow_loss"] < 1e-5             # (the soft forward test's bounds for the predictor)


def test_graphed_forward_replays_the_eager_forward(hard_model, fixture_and_inputs):
    """The hard-duration forward captures as one HIP graph (MAS on the main stream, the flow predictor beside the decoder)."""
    _, inp = fixture_and_inputs
    eager = hard_model(**inp)
    gf = graph.GraphedForward(hard_model, **inp)
    out = gf(**{k: inp[k] for k in ("text", "mel", "pitch", "energy")})
    torch.cuda.synchronize()
    assert torch.equal(out.mel, eager.mel) and torch.equal(out.adaptor_output.dec_lengths, eager.adaptor_output.dec_lengths)
    assert torch.equal(out.adaptor_output.losses["flow_loss"], eager.adaptor_output.losses["flow_loss"])
    with pytest.raises(NotImplementedError, match="MAS durations"):
        graph.SegmentedForward(hard_model, *(inp[k] for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy")))


def test_infer_against_the_reference_fixture(hard_model, fixture_and_inputs):
    g, inp = fixture_and_inputs
    assert float(g["infer_margin"]) >= 1e-3
    for tag, sl, text_len in (("b2", slice(None), inp["text_len"]), ("b1", slice(0, 1), None)):
        mel, ao = hard_model.infer(inp["text"][sl], text_lengths=text_len, steps=4, flow_noise=inp["flow_noise"][sl])
        torch.cuda.synchronize()
        assert np.array_equal(ao.duration.cpu().numpy(), g[f"{tag}_duration"]), tag
        assert np.array_equal(ao.dec_lengths.cpu().numpy(), g[f"{tag}_dec_lengths"]), tag
        assert mel.shape == g[f"{tag}_mel"].shape
        d = _maxdiff(mel, g[f"{tag}_mel"])
        print(f"hard-duration infer {tag}: mel vs reference {d:.2e}, {mel.shape[2]} frames")
        assert d <= MEL_TOL + float(g["d_mel"]), tag
        assert _maxdiff(ao.pitch, g[f"{tag}_pitch"]) < MEL_TOL and _maxdiff(ao.energy, g[f"{tag}_energy"]) < MEL_TOL


def test_bf16_infer_with_the_fixture_durations(hard_model, fixture_and_inputs):
    """bf16 compute path: the predictions move, so the fixture's durations are passed as the target (the shapes then agree);
    held to the bound the soft bf16 `infer` test states."""
    g, inp = fixture_and_inputs
    dur = torch.from_numpy(g["b2_duration"]).to(DEV)
    ref = torch.from_numpy(g["b2_mel"]).double()
    try:
        hard_model.set_compute_dtype(torch.bfloat16)
        mel, ao = hard_model.infer(inp["text"], text_lengths=inp["text_len"], duration_target=dur, steps=4,
                                   flow_noise=inp["flow_noise"], max_dec_len=ref.shape[2])
        torch.cuda.synchronize()
    finally:
        hard_model.set_compute_dtype(torch.float32)
    assert np.array_equal(ao.dec_lengths.cpu().numpy(), g["b2_dec_lengths"]) and mel.shape == ref.shape
    e = mel.cpu().double() - ref
    linf, rel = float(e.abs().max()), float(e.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"hard-duration bf16 infer: mel L-inf {linf:.2e}, relative RMS {rel:.2e}")
    assert linf < INFER_BF16_MEL_TOL and rel < 3e-2


def test_infer_with_a_given_length_captures_in_a_graph(hard_model, fixture_and_inputs):
    _, inp = fixture_and_inputs
    kw = dict(text_lengths=inp["text_len"], steps=4, flow_noise=inp["flow_noise"], max_dec_len=64)
    mel, ao = hard_model.infer(inp["text"], **kw)
    g = graph.GraphedCall(lambda: hard_model.infer(inp["text"], **kw))
    mel_g, ao_g = g.replay()
    torch.cuda.synchronize()
    assert mel.shape == (2, 80, 64) and torch.equal(mel_g, mel) and torch.equal(ao_g.dec_lengths, ao.dec_lengths)
    assert torch.equal(ao_g.duration, ao.duration) and not mel[0, :, 56:].any()


# ------------------------------------------------------------------------------------------------------------ training
def _trainable(state_dict):
    model = AcousticModel.init(AcousticDims().model_config(soft_duration=False))
    model.load_state_dict(state_dict, strict=True)
    return model.to(DEV).eval()


def _sample(t, n=192):
    f = t.detach().reshape(-1)
    return f[::max(1, -(-f.numel() // n))].cpu()


def test_training_step_against_the_reference_fixture(state_dict, fixture_and_inputs):
    """The hard-duration step against the reference's own (tools/make_hard_duration_goldens.py `gen_train`) with train.npz's
    tolerances: the four losses to 2e-4, all 206 gradients - norm and strided sample - to 2e-3 of the tensor's scale."""
    g, inp = fixture_and_inputs
    model = _trainable(state_dict)
    names = [str(n) for n in g["names"]]
    params = dict(model.named_parameters())
    assert list(params) == names and len(names) == 206
    _, total, losses = train.acoustic_train_forward(model, inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"],
                                                    inp["energy"], flow_noise=inp["flow_noise"], flow_time=inp["flow_time"],
                                                    train_aligner=True)
    for k, v in losses.items():
        ref = float(g["loss_" + k.replace("/", "_")])
        assert abs(v.item() - ref) < 2e-4 * max(abs(ref), 1.0), (k, v.item(), ref)
    assert abs(total.item() - float(g["loss_total"])) < 2e-4 * float(g["loss_total"])
    total.backward()
    worst = 0.0
    for i, n in enumerate(names):
        gr, scale = params[n].grad, float(g["grad_absmax"][i])
        assert gr is not None, n
        assert abs(gr.double().norm().item() - float(g["grad_norm"][i])) <= 2e-3 * float(g["grad_norm"][i]) + 1e-7, n
        err = (_sample(gr) - torch.from_numpy(g[f"g{i}"])).abs().max().item() / max(scale, 1e-12)
        worst = max(worst, err)
        assert err <= 2e-3, (n, err)
    print(f"hard-duration HIP backward vs the reference's gradients: worst sampled error = {worst:.2e} of the tensor's scale")


def test_mel_loss_alone_leaves_the_aligner_without_a_gradient(state_dict, fixture_and_inputs):
    """With hard durations nothing but the CTC and binarisation terms reaches the aligner (the reference leaves `grad is None`)."""
    _, inp = fixture_and_inputs
    model = _trainable(state_dict)
    out = train.acoustic_train_outputs(model, inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"], inp["energy"],
                                       inp["flow_noise"], inp["flow_time"])
    train.MelLoss()(out.mel, inp["mel"], inp["mel_len"]).backward()
    aligner = list(model.aligner.parameters())
    assert aligner and all(p.grad is None or not p.grad.any() for p in aligner)
    assert all(p.grad is not None and bool(p.grad.any()) for p in model.decoder.parameters())
    assert bool(model.text_embedding.weight.grad.any()) and bool(model.temporal_adaptor.embedding.linear_layer.weight.grad.any())


def test_graphed_training_step_replays_match_eager_steps(state_dict):
    """train.GraphedTrainStep, unchanged, on a hard-duration model: replays give bit for bit the parameters of the same number of
    eager steps (the pattern of tests/test_gpu_train.py's test of that name)."""
    def make():
        torch.manual_seed(11)
        m = _trainable(state_dict)
        o = train.FlatAdamW(list(m.parameters()), lr=2e-4, weight_decay=1e-2, grad_clip=1.0)
        o.check_finite = False
        return m, o
    d = {k: v.to(DEV) for k, v in synth.make_inputs(3, 52, 160, variable=True, seed=9).items()}
    batch = {k: d[k] for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy", "flow_x0", "flow_t")}
    m_e, o_e = make()
    eager_tot = []
    for _ in range(4):
        _, total, _ = train.acoustic_train_forward(m_e, d["text"], d["text_len"], d["mel"], d["mel_len"], d["pitch"], d["energy"],
                                                   flow_noise=d["flow_x0"], flow_time=d["flow_t"], amp=True)
        o_e.step(total)
        eager_tot.append(float(total.detach()))
    m_g, o_g = make()
    step = train.GraphedTrainStep(m_g, o_g, batch, amp=True, warmup=2)        # two real steps ...
    graph_tot = [float(step(**batch)[0].detach()) for _ in range(2)]          # ... and two replays = four steps
    torch.cuda.synchronize()
    assert o_g.step_count == 4 and o_e.step_count == 4
    assert graph_tot == eager_tot[2:], f"losses: graph {graph_tot} vs eager {eager_tot[2:]}"
    assert torch.equal(o_g.flat.data, o_e.flat.data) and torch.equal(o_g.exp_avg_sq, o_e.exp_avg_sq)
    assert eager_tot[-1] < eager_tot[0]
