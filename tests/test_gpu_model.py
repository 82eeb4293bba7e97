"""GPU parity of the module mirror (Attention, FeedForward, TransformerLayer, Transformer, AcousticModel.forward/infer)
against the golden fixtures generated from the real reference, and against the oracle on other seeded inputs.

Tolerances: BASELINE.json's bar is mel L-inf < 1e-4 (fp32); per-op outputs are held to 5e-5."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from conftest import crc, golden

pytestmark = pytest.mark.gpu

from isp_tts_amd import runtime, synth  # noqa: E402
from isp_tts_amd.modules.transformer import plan  # noqa: E402
from oracle import acoustic_oracle as orc  # noqa: E402

DEV = "cuda"
OP_TOL = 5e-5
MEL_TOL = 1e-4


def _maxdiff(a, b):
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a)
    b = b.detach().cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.double() - b.double()).abs().max().item()


@pytest.mark.parametrize("tag,n", [("enc", 100), ("dec", 512)])
def test_ops_against_reference_goldens(gpu_model, tag, n):
    g = golden("ops.npz")
    step = int(g[f"{tag}_row_step"])
    lens = torch.tensor(g[f"{tag}_lens"])
    x = synth._normal(f"golden/op/{tag}/x", (2, n, 384))
    assert crc(x) == int(g[f"{tag}_x_crc"])
    mask = (torch.arange(n)[None] < lens[:, None]).to(DEV)
    xd = x.to(DEV)
    stack = gpu_model.encoder if tag == "enc" else gpu_model.decoder
    layer = stack.layers[0]
    out, inter, shared = layer.attention(xd, mask=mask)
    assert _maxdiff(out[:, ::step], g[f"{tag}_attention"]) < OP_TOL
    assert inter.queries.shape == (2, 6, n, 64) and inter.keys.shape == (2, n, 64) and shared.rel_pos_bias is None
    assert _maxdiff(layer.attention(xd)[0][:, ::step], g[f"{tag}_attention_nomask"]) < OP_TOL
    assert _maxdiff(layer.feed_forward(xd)[:, ::step], g[f"{tag}_feed_forward"]) < OP_TOL
    assert _maxdiff(layer(xd, mask=mask).out[:, ::step], g[f"{tag}_layer"]) < OP_TOL
    assert _maxdiff(stack(xd, mask=mask).out[:, ::step], g[f"{tag}_transformer"]) < OP_TOL
    assert _maxdiff(stack(xd).out[:, ::step], g[f"{tag}_transformer_nomask"]) < OP_TOL


def test_decoder_stack_at_the_data_bound_of_1723_frames(gpu_model, state_dict):
    """The recipes admit utterances up to 1,723 mel frames (recipes/acoustic/core.yaml:33-47): the MelDecoder
    stack (6 layers, ALiBi distances up to 1,722) on B = 2 ragged rows at that length against the oracle's `transformer` - the
    exact-fp32 and split-fp16 paths to the per-op bar scaled by the output's size, the bf16 path to its stated bound."""
    n, lens = 1723, torch.tensor([1723, 1289])
    x = synth._normal("t/stack1723/x", (2, n, 384))
    mask = torch.arange(n)[None] < lens[:, None]
    ref = orc.transformer(state_dict, "decoder", x, mask)
    scale = float(ref.abs().max())
    xd, md, ld = x.to(DEV), mask.to(DEV), lens.to(DEV)
    dec = gpu_model.decoder
    try:
        for dtype, tol in ((torch.float32, OP_TOL), (torch.float16, OP_TOL), (torch.bfloat16, 6e-2)):
            dec.set_compute_dtype(dtype)
            out = dec(xd, mask=md, key_len=ld).out
            err = _maxdiff(out, ref)
            print(f"decoder stack at 1723 frames, {dtype}: L-inf {err:.2e} (|out| <= {scale:.1f})")
            assert err < tol * max(1.0, scale), (dtype, err)
            assert float(out[1, 1289:].abs().max()) == 0.0          # padded rows are exactly zero
    finally:
        dec.set_compute_dtype(torch.float32)


def test_adaptive_norm_stack_against_reference_goldens(gpu_model):
    g = golden("ops.npz")
    n, lens = 100, torch.tensor(g["ada_lens"])
    x = synth._normal("golden/op/ada/x", (2, n, 387))
    assert crc(x) == int(g["ada_x_crc"])
    cond = synth._normal("golden/op/ada/cond", (2, 32)).to(DEV)
    mask = (torch.arange(n)[None] < lens[:, None]).to(DEV)
    tr = gpu_model.temporal_adaptor.predictor.transformer
    assert _maxdiff(tr(x.to(DEV), mask=mask, adaptive_condition=cond).out, g["ada_transformer"]) < OP_TOL
    x256 = synth._normal("golden/op/ada/x256", (2, n, 256)).to(DEV)
    assert _maxdiff(tr.layers[0](x256, mask=mask, adaptive_condition=cond).out, g["ada_layer"]) < OP_TOL
    cond3 = synth._normal("golden/op/ada/cond3", (1, 1, 32)).to(DEV)
    assert _maxdiff(tr(x.to(DEV), mask=mask, adaptive_condition=cond3).out, g["ada_transformer_cond3"]) < OP_TOL


def _forward_inputs():
    inp = synth.make_inputs(2, 100, 512)
    text_len, mel_len = torch.tensor([100, 73]), torch.tensor([512, 390])
    tm = torch.arange(100)[None] < text_len[:, None]
    mm = torch.arange(512)[None] < mel_len[:, None]
    return dict(text=inp["text"] * tm, text_len=text_len, mel=inp["mel"] * mm[:, None], mel_len=mel_len,
                pitch=inp["pitch"] * mm, energy=inp["energy"] * mm, flow_noise=inp["flow_x0"], flow_time=inp["flow_t"])


def test_forward_against_reference_golden(gpu_model):
    g = golden("forward.npz")
    inp = _forward_inputs()
    assert [crc(inp[k]) for k in ("text", "mel", "pitch", "energy")] == [int(v) for v in g["inputs_crc"]]
    out = gpu_model(**{k: v.to(DEV) for k, v in inp.items()})
    torch.cuda.synchronize()
    assert out.mel.shape == (2, 80, 512)
    d = _maxdiff(out.mel, g["mel"])
    print(f"forward mel L-inf vs reference = {d:.3e}")
    assert d < MEL_TOL
    assert np.array_equal(out.adaptor_output.dec_lengths.cpu().numpy(), g["dec_lengths"])
    diffs = {"attn_logits": _maxdiff(out.aligner_output.attn_logits, g["attn_logits"]),
             "attn_soft": _maxdiff(out.aligner_output.attn_soft[:, ::8], g["attn_soft_rows"]),
             "log_duration": _maxdiff(out.adaptor_output.log_duration, g["log_duration"]),
             "pitch": _maxdiff(out.adaptor_output.pitch, g["pitch"]),
             "pitch_target": _maxdiff(out.adaptor_output.pitch_target, g["pitch_target"]),
             "flow_loss": abs(float(out.adaptor_output.losses["flow_loss"]) - float(g["flow_loss"]))}
    print("forward vs reference: " + ", ".join(f"{k} {v:.2e}" for k, v in diffs.items()))
    assert diffs["attn_logits"] < 2e-4        # HIP front-end (fp32 MFMA convolutions); logits reach down to -35
    assert diffs["attn_soft"] < 2e-5
    assert diffs["log_duration"] < 1e-4 and diffs["pitch"] < 1e-4
    assert diffs["pitch_target"] < 2e-5
    assert diffs["flow_loss"] < 1e-5
    # MAS on the reference's own pre-MAS logits is bit-exact (the end-to-end path may differ at near-ties because the
    # front-end logits differ in the last bits, SURVEY 7 "MAS bit-exactness")
    hard = gpu_model.aligner.binarize_attention_parallel(torch.from_numpy(g["attn_logits"]).to(DEV),
                                                         inp["text_len"].to(DEV), inp["mel_len"].to(DEV))
    path = g["path"]
    ref_hard = np.zeros(hard.shape, np.int16)
    bi, mi = np.nonzero(path >= 0)
    ref_hard[bi, mi, path[bi, mi]] = 1
    assert hard.dtype == torch.int16 and np.array_equal(hard.cpu().numpy(), ref_hard)
    assert np.array_equal(out.aligner_output.attn_hard_duration.sum(1).cpu().numpy(), g["mel_len"])


def test_infer_against_reference_golden(gpu_model):
    g = golden("infer.npz")
    inp = synth.make_inputs(2, 100, 512)
    text_len = torch.tensor(g["b2_text_len"])
    text = (inp["text"] * (torch.arange(100)[None] < text_len[:, None])).to(DEV)
    dur = torch.from_numpy(g["b2_dur"]).to(DEV)
    x_t = inp["flow_x0"].to(DEV)
    mel, ao = gpu_model.infer(text, text_lengths=text_len.to(DEV), duration_target=dur, steps=4, flow_noise=x_t)
    assert _maxdiff(mel, g["b2_mel"]) < MEL_TOL
    assert _maxdiff(ao.pitch, g["b2_pitch"]) < MEL_TOL and _maxdiff(ao.energy, g["b2_energy"]) < MEL_TOL
    assert np.array_equal(ao.dec_lengths.cpu().numpy(), g["b2_dec_lengths"])
    # single utterance: no masks anywhere
    mel1, ao1 = gpu_model.infer(text[:1], duration_target=dur[:1], steps=4, flow_noise=x_t[:1])
    assert _maxdiff(mel1, g["b1_mel"]) < MEL_TOL
    # predicted (fractional) durations
    melp, aop = gpu_model.infer(text, text_lengths=text_len.to(DEV), steps=4, flow_noise=x_t)
    assert _maxdiff(aop.duration, g["b2p_duration"]) < 1e-3
    # the decoder lengths are floor(sum of fractional durations + 0.5): asserted, not assumed (an fp32-noisy sum that lands
    # on the other side of x.5 would change the output SHAPE - it does not on these fixtures)
    assert np.array_equal(aop.dec_lengths.cpu().numpy(), g["b2p_dec_lengths"])
    assert _maxdiff(melp, g["b2p_mel"]) < 5e-4       # soft path is continuous in the (fp32-noisy) predicted durations


def test_multi_speaker_infer_against_reference_golden(state_dict):
    """Row f3: a multi-speaker model (model.py:93-97; the authors' published checkpoint has 1,307 speakers) through `infer` with
    speaker ids (:205-207) against outputs of the reference itself (tests/golden/infer_speakers.npz): the collator's [B, 1]
    field and a single id; fp32, split-fp16 (1e-4) and bf16 (its stated infer bound)."""
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    g = golden("infer_speakers.npz")
    sd = dict(state_dict)
    sd["speaker_embedding.weight"] = synth.make_speaker_table(4)
    model = AcousticModel.init(dict(AcousticDims().model_config(), num_speakers=4)).eval()
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    inp = synth.make_inputs(2, 100, 512)
    text_len = torch.tensor(g["b2_text_len"])
    text = (inp["text"] * (torch.arange(100)[None] < text_len[:, None])).to(DEV)
    dur = torch.from_numpy(g["b2_dur"]).to(DEV)
    x_t = inp["flow_x0"].to(DEV)
    spk2, spk1 = torch.from_numpy(g["b2_speaker"]).to(DEV), torch.from_numpy(g["b1_speaker"]).to(DEV)
    for dtype, tol in ((torch.float32, MEL_TOL), (torch.float16, MEL_TOL), (torch.bfloat16, 2e-1)):
        model.set_compute_dtype(dtype)
        mel, ao = model.infer(text, text_lengths=text_len.to(DEV), duration_target=dur, steps=4, flow_noise=x_t, speaker=spk2)
        assert _maxdiff(mel, g["b2_mel"]) < tol, dtype
        assert _maxdiff(ao.pitch, g["b2_pitch"]) < tol and _maxdiff(ao.energy, g["b2_energy"]) < tol
        assert np.array_equal(ao.dec_lengths.cpu().numpy(), g["b2_dec_lengths"])
        mel1, _ = model.infer(text[:1], duration_target=dur[:1], steps=4, flow_noise=x_t[:1], speaker=spk1)
        assert _maxdiff(mel1, g["b1_mel"]) < tol, dtype
    model.set_compute_dtype(torch.float32)
    plain, _ = model.infer(text, text_lengths=text_len.to(DEV), duration_target=dur, steps=4, flow_noise=x_t)     # speaker=None: no add
    assert _maxdiff(plain, g["b2_mel"]) > 0.1
    with pytest.raises(ValueError):      # [B] ids with B > 1 do not broadcast in the reference either
        model.infer(text, text_lengths=text_len.to(DEV), duration_target=dur, steps=4, flow_noise=x_t, speaker=torch.tensor([3, 1], device=DEV))
    with pytest.raises(AttributeError, match="speaker_encoder"):   # model.py:145-146
        model(text, text_len.to(DEV), inp["mel"].to(DEV), inp["mel_len"].to(DEV), inp["pitch"].to(DEV), inp["energy"].to(DEV), speaker=spk2)


def test_predictor_head_in_one_pass_equals_the_three_launches(gpu_model):
    """`ispk_flow_head_f32` (final LayerNorm of the predictor's stack + linear_layer + flow-matching algebra per row, block partials
    added in a fixed order) against the three launches it replaces (LayerNorm, linear_small, flow_finish): same values to fp32
    summation order, masked positions exactly zero, deterministic; ragged lengths, L not a multiple of the 16-row blocks."""
    inp = synth.make_inputs(5, 53, 160, variable=True, seed=13)
    args = [inp[k].to(DEV) for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy")]
    kw = dict(flow_noise=inp["flow_x0"].to(DEV), flow_time=inp["flow_t"].to(DEV))
    pred = gpu_model.temporal_adaptor.predictor
    assert pred.fused_head
    a = gpu_model(*args, **kw).adaptor_output
    a2 = gpu_model(*args, **kw).adaptor_output
    try:
        pred.fused_head = False
        b = gpu_model(*args, **kw).adaptor_output
    finally:
        pred.fused_head = True
    for name in ("log_duration", "pitch", "energy", "duration"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, getattr(a2, name)), name
        assert _maxdiff(x, y) < 2e-6 * max(1.0, float(y.abs().max())), name
    assert abs(float(a.losses["flow_loss"]) - float(b.losses["flow_loss"])) < 2e-6 * float(b.losses["flow_loss"])
    tmask = (torch.arange(53)[None] < inp["text_len"][:, None]).to(DEV)
    assert float((a.log_duration * ~tmask).abs().max()) == 0.0 and float((a.pitch * ~tmask).abs().max()) == 0.0


def test_forward_matches_oracle_on_other_inputs(gpu_model, state_dict):
    """Different seed, B=3 variable lengths (not in the fixtures): HIP path vs the oracle."""
    inp = synth.make_inputs(3, 60, 200, variable=True, seed=7)
    args = (inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"], inp["energy"])
    ref = orc.acoustic_forward(state_dict, *args, inp["flow_x0"], inp["flow_t"])
    out = gpu_model(*[a.to(DEV) for a in args], flow_noise=inp["flow_x0"].to(DEV), flow_time=inp["flow_t"].to(DEV))
    assert _maxdiff(out.mel, ref.mel) < MEL_TOL
    assert np.array_equal(out.adaptor_output.dec_lengths.cpu().numpy(), ref.adaptor.dec_lengths.numpy())


def test_full_size_forward_properties(gpu_model):
    """BASELINE headline size (B=64, L=100, M=512): padding invariance and batch independence."""
    inp = synth.make_inputs(64, 100, 512, variable=True)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    kw = dict(flow_noise=dev["flow_x0"], flow_time=dev["flow_t"])
    out = gpu_model(dev["text"], dev["text_len"], dev["mel"], dev["mel_len"], dev["pitch"], dev["energy"], **kw)
    assert out.mel.shape == (64, 80, 512) and torch.isfinite(out.mel).all()
    mm = torch.arange(512, device=DEV)[None] < dev["mel_len"][:, None]
    assert (out.mel * ~mm[:, None]).abs().max() == 0, "padded frames must be exactly zero"
    assert torch.equal(out.aligner_output.attn_hard_duration.sum(1), dev["mel_len"])
    # an utterance's mel does not depend on its batch neighbours
    sub = slice(5, 9)
    out4 = gpu_model(dev["text"][sub], dev["text_len"][sub], dev["mel"][sub], dev["mel_len"][sub], dev["pitch"][sub],
                     dev["energy"][sub], flow_noise=dev["flow_x0"][sub], flow_time=dev["flow_t"][sub])
    assert _maxdiff(out4.mel, out.mel[sub]) < 2e-5


# ------------------------------------------------------------------------------------------------ bf16 throughput path
INFER_BF16_MEL_TOL = 2e-1   # infer on the bf16 path: predicted prosody through bf16 stacks into the decoder (stated, measured 1.1e-1)
BF16_MEL_TOL = 6e-2   # bf16 operands (8 mantissa bits) through 12 layers, fp32 residual stream; stated, not the 1e-4 bar


def test_bf16_forward_error_vs_reference(gpu_model):
    """The bf16 path (BASELINE config 3 dtype) against the fp32 reference golden: reported and bounded, NOT held to 1e-4."""
    g = golden("forward.npz")
    inp = _forward_inputs()
    try:
        gpu_model.set_compute_dtype(torch.bfloat16)
        out = gpu_model(**{k: v.to(DEV) for k, v in inp.items()})
        torch.cuda.synchronize()
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    ref = torch.from_numpy(g["mel"])
    err = (out.mel.cpu() - ref).abs()
    rel_rms = (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"bf16 forward: mel L-inf = {err.max().item():.3e}, relative RMS = {rel_rms:.3e}")
    assert err.max().item() < BF16_MEL_TOL and rel_rms < 1e-2
    assert np.array_equal(out.adaptor_output.dec_lengths.cpu().numpy(), g["dec_lengths"])
    # back on the fp32 path the 1e-4 bar holds again (staged weights are rebuilt per dtype)
    out = gpu_model(**{k: v.to(DEV) for k, v in inp.items()})
    assert _maxdiff(out.mel, g["mel"]) < MEL_TOL


@pytest.fixture(scope="module")
def headline_case(state_dict):
    """BASELINE config 3 itself: B=64 x L=100 x M=512 (variable lengths inside the padded shape, so masks are live), the
    oracle's outputs for it (about 3 s on the GPU box's host cores), computed once for the tests below."""
    inp = synth.make_inputs(64, 100, 512, variable=True)
    args = (inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"], inp["energy"])
    ref = orc.acoustic_forward(state_dict, *args, inp["flow_x0"], inp["flow_t"])
    return inp, ref


def _run_headline(gpu_model, inp):
    dev = {k: v.to(DEV) for k, v in inp.items()}
    out = gpu_model(dev["text"], dev["text_len"], dev["mel"], dev["mel_len"], dev["pitch"], dev["energy"],
                    flow_noise=dev["flow_x0"], flow_time=dev["flow_t"])
    torch.cuda.synchronize()
    return out


def _identical_paths(a, b) -> int:
    return int((a.cpu() == b.cpu()).flatten(1).all(1).sum())


def test_headline_config_fp32_path_against_the_oracle(gpu_model, headline_case):
    """B=64 x 100 x 512, fp32 path vs the oracle: the north-star bars at the benchmark configuration itself."""
    inp, ref = headline_case
    out = _run_headline(gpu_model, inp)
    d = _maxdiff(out.mel, ref.mel)
    print(f"B=64 fp32: mel L-inf vs oracle = {d:.3e}")
    assert d < MEL_TOL
    assert torch.equal(out.adaptor_output.dec_lengths.cpu(), ref.adaptor.dec_lengths)
    assert _maxdiff(out.aligner_output.attn_soft, ref.aligner.attn_soft) < 1e-4
    # MAS at its boundary: the kernel on the ORACLE's pre-MAS logits is bit-exact on all 64 utterances ...
    hard = gpu_model.aligner.binarize_attention_parallel(ref.aligner.attn_logits.to(DEV), inp["text_len"].to(DEV),
                                                         inp["mel_len"].to(DEV))
    assert torch.equal(hard.cpu(), ref.aligner.attn_hard)
    # ... and end to end (own fp32 front-end logits, which differ from the oracle's in the last bits) reported:
    same = _identical_paths(out.aligner_output.attn_hard, ref.aligner.attn_hard)
    print(f"B=64 fp32: {same}/64 end-to-end alignments identical to the oracle's")
    assert same >= 60 and torch.equal(out.aligner_output.attn_hard_duration.sum(1).cpu(), inp["mel_len"])


def test_headline_config_split_fp16_path_against_the_oracle(gpu_model, headline_case):
    """The parity-grade FAST path (`set_compute_dtype(torch.float16)`: every product three fp16 MFMAs over hi / lo terms,
    csrc/split.hip) at the benchmark configuration: the same north-star bars as the exact-fp32 path - mel L-inf < 1e-4 and
    the oracle's MAS alignments on all 64 utterances."""
    inp, ref = headline_case
    try:
        gpu_model.set_compute_dtype(torch.float16)
        out = _run_headline(gpu_model, inp)
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    d = _maxdiff(out.mel, ref.mel)
    dl = _maxdiff(out.aligner_output.attn_logits, ref.aligner.attn_logits)
    same = _identical_paths(out.aligner_output.attn_hard, ref.aligner.attn_hard)
    print(f"B=64 split-fp16: mel L-inf vs oracle = {d:.3e}, attn_logits {dl:.3e}, {same}/64 alignments identical to the oracle's")
    assert d < MEL_TOL
    assert torch.equal(out.adaptor_output.dec_lengths.cpu(), ref.adaptor.dec_lengths)
    assert _maxdiff(out.aligner_output.attn_soft, ref.aligner.attn_soft) < 1e-4
    assert same == 64
    assert torch.equal(out.aligner_output.attn_hard_duration.cpu(), ref.aligner.attn_hard_duration)


def test_headline_config_bf16_path_against_the_oracle(gpu_model, headline_case):
    """The benchmarked configuration (bf16 operands in every stack and in the aligner front-end) against the ORACLE on all 64
    utterances - mel does not depend on the hard alignment (the decoder input is built from `attn_soft` and the dense
    targets, temporal_adaptor.py:284-300), so no utterance is filtered out.  bf16 operands (8 mantissa bits) through 12
    layers with an fp32 residual stream: the bound is stated here, it is NOT the 1e-4 bar (that is the fp32 path's)."""
    inp, ref = headline_case
    try:
        gpu_model.set_compute_dtype(torch.bfloat16)
        out = _run_headline(gpu_model, inp)
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    err = (out.mel.cpu() - ref.mel).abs()
    rel_rms = (err.pow(2).mean().sqrt() / ref.mel.pow(2).mean().sqrt()).item()
    same = _identical_paths(out.aligner_output.attn_hard, ref.aligner.attn_hard)
    print(f"B=64 bf16: mel L-inf vs oracle = {err.max().item():.3e}, relative RMS = {rel_rms:.3e}; {same}/64 alignments "
          f"identical to the oracle's (bf16 alignment chain)")
    assert err.max().item() < BF16_MEL_TOL and rel_rms < 1e-2
    mm = torch.arange(512)[None] < inp["mel_len"][:, None]
    assert (out.mel.cpu() * ~mm[:, None]).abs().max() == 0 and torch.isfinite(out.mel).all()
    assert torch.equal(out.adaptor_output.dec_lengths.cpu(), ref.adaptor.dec_lengths)
    assert torch.equal(out.aligner_output.attn_hard_duration.sum(1).cpu(), inp["mel_len"])


def test_headline_config_bf16_with_fp32_alignment_chain_has_the_fp32_paths(gpu_model, headline_case):
    """`set_compute_dtype(bf16, alignment_dtype=fp32)`: everything upstream of MAS (text encoder, aligner front-end) runs
    the fp32 path's kernels, so logits, hard alignments and durations are BIT-IDENTICAL to the fp32 path's on all 64
    utterances, while the decoder and the adaptor stacks stay bf16 (mel within the bf16 bound)."""
    inp, ref = headline_case
    ref32 = _run_headline(gpu_model, inp)
    try:
        gpu_model.set_compute_dtype(torch.bfloat16, alignment_dtype=torch.float32)
        out = _run_headline(gpu_model, inp)
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    assert torch.equal(out.aligner_output.attn_logits, ref32.aligner_output.attn_logits)
    assert torch.equal(out.aligner_output.attn_hard, ref32.aligner_output.attn_hard)          # all 64, no filter
    assert torch.equal(out.aligner_output.attn_hard_duration, ref32.aligner_output.attn_hard_duration)
    err = (out.mel.cpu() - ref.mel).abs()
    print(f"B=64 bf16 + fp32 alignment chain: mel L-inf vs oracle = {err.max().item():.3e}")
    assert err.max().item() < BF16_MEL_TOL


def test_headline_config_bf16_with_split_fp16_alignment_chain_has_the_oracle_paths(gpu_model, headline_case):
    """`set_compute_dtype(bf16, alignment_dtype=torch.float16)`: the chain upstream of MAS (text encoder, aligner front-end)
    on split-fp16 products - fp32-grade logits at a third of the exact-fp32 chain's cost - under the bf16 decoder / adaptor:
    all 64 hard alignments and durations equal the ORACLE's, mel within the bf16 bound."""
    inp, ref = headline_case
    try:
        gpu_model.set_compute_dtype(torch.bfloat16, alignment_dtype=torch.float16)
        out = _run_headline(gpu_model, inp)
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    same = _identical_paths(out.aligner_output.attn_hard, ref.aligner.attn_hard)
    err = (out.mel.cpu() - ref.mel).abs().max().item()
    print(f"B=64 bf16 + split-fp16 alignment chain: {same}/64 alignments identical to the oracle's, mel L-inf {err:.3e}")
    assert same == 64 and torch.equal(out.aligner_output.attn_hard_duration.cpu(), ref.aligner.attn_hard_duration)
    assert _maxdiff(out.aligner_output.attn_logits, ref.aligner.attn_logits) < 5e-4
    assert err < BF16_MEL_TOL


@pytest.mark.parametrize("which", ["longest", "shortest"])
def test_config4_shapes_against_the_oracle(gpu_model, state_dict, which):
    """BASELINE config 4 shapes (B=256, 128..1024 frames, up to 200 tokens, sharded over 8 ranks): the micro-batch rank 0
    (few long utterances, M_pad = 1024, L_pad = 200) and the one the last rank (many short ones) really run, cut by the
    same planner bench.py uses, through `forward` - fp32 against the oracle at the 1e-4 bar, bf16 at its stated bound."""
    from isp_tts_amd import dist as idist
    full = synth.make_inputs(256, 200, 1024, variable=True)
    _, plans = idist.plan_micro_batches(full["mel_len"].tolist(), full["text_len"].tolist(), 8)
    idx, m_pad, l_pad = plans[0][0] if which == "longest" else plans[7][-1]
    # bounded oracle time; the micro-batch's longest member stays in, so the padded shape is the plan's
    idx = idx[:12] if which == "longest" else idx[:8] + idx[-32:]
    ii = torch.tensor(idx)
    mb = {"text": full["text"][ii, :l_pad], "text_len": full["text_len"][ii], "mel": full["mel"][ii, :, :m_pad],
          "mel_len": full["mel_len"][ii], "pitch": full["pitch"][ii, :m_pad], "energy": full["energy"][ii, :m_pad],
          "flow_x0": full["flow_x0"][ii, :l_pad], "flow_t": full["flow_t"][ii]}
    if which == "longest":
        assert m_pad == 1024 and l_pad == 200
    # the oracle (like the reference) sizes its masks by the longest member; the planner rounds the padded shape up to
    # multiples of 8 frames / 4 tokens, so the oracle gets the exact maxima and the extra padding must come out as zeros
    mx, lx = int(mb["mel_len"].max()), int(mb["text_len"].max())
    assert 0 <= m_pad - mx < 8 and 0 <= l_pad - lx < 4
    ref = orc.acoustic_forward(state_dict, mb["text"][:, :lx], mb["text_len"], mb["mel"][:, :, :mx], mb["mel_len"],
                               mb["pitch"][:, :mx], mb["energy"][:, :mx], mb["flow_x0"][:, :lx], mb["flow_t"])
    out = _run_headline(gpu_model, mb)
    assert out.mel.shape[2] == m_pad and (out.mel[:, :, mx:] == 0).all()
    d = _maxdiff(out.mel[:, :, :mx], ref.mel)
    print(f"config 4 ({which}: {len(idx)} x M={m_pad} x L={l_pad}) fp32: mel L-inf vs oracle = {d:.3e}")
    assert d < MEL_TOL and torch.equal(out.adaptor_output.dec_lengths.cpu(), ref.adaptor.dec_lengths)
    hard = gpu_model.aligner.binarize_attention_parallel(ref.aligner.attn_logits.to(DEV), mb["text_len"].to(DEV),
                                                         mb["mel_len"].to(DEV))
    assert torch.equal(hard.cpu(), ref.aligner.attn_hard)
    # the parity-grade fast path (split-fp16 products) on the same micro-batch: the 1e-4 bar and the oracle's alignments
    try:
        gpu_model.set_compute_dtype(torch.float16)
        outs = _run_headline(gpu_model, mb)
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    ds = _maxdiff(outs.mel[:, :, :mx], ref.mel)
    same = _identical_paths(outs.aligner_output.attn_hard[:, :mx, :lx], ref.aligner.attn_hard)
    print(f"config 4 ({which}) split-fp16: mel L-inf vs oracle = {ds:.3e}, {same}/{len(idx)} alignments identical to the oracle's")
    assert ds < MEL_TOL and same == len(idx) and torch.equal(outs.adaptor_output.dec_lengths.cpu(), ref.adaptor.dec_lengths)
    try:
        gpu_model.set_compute_dtype(torch.bfloat16)
        out16 = _run_headline(gpu_model, mb)
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    e16 = (out16.mel.cpu()[:, :, :mx] - ref.mel).abs().max().item()
    print(f"config 4 ({which}) bf16: mel L-inf vs oracle = {e16:.3e}")
    assert e16 < BF16_MEL_TOL and torch.equal(out16.adaptor_output.dec_lengths.cpu(), ref.adaptor.dec_lengths)
    mm = torch.arange(m_pad)[None] < mb["mel_len"][:, None]
    assert (out16.mel.cpu() * ~mm[:, None]).abs().max() == 0


def test_forward_issues_no_aten_compute_ops(gpu_model):
    """Everything `AcousticModel.forward` computes is a libispk launch: embedding lookup, masks, time embedding, duration
    fix-up, length regulation and the flow loss included.  A TorchDispatchMode sees only
    views and allocations - no element-wise, reduction, cat, bmm or copy kernel of PyTorch's own."""
    from torch.utils._python_dispatch import TorchDispatchMode
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not str(func).startswith(harmless):
                seen.append(str(func))
            return func(*args, **(kwargs or {}))

    inp = {k: v.to(DEV) for k, v in _forward_inputs().items()}
    for dtype in (torch.float32, torch.bfloat16):
        try:
            gpu_model.set_compute_dtype(dtype)
            gpu_model(**inp)            # stages weights (casts, packing) outside the traced call
            with Spy():
                gpu_model(**inp)
        finally:
            gpu_model.set_compute_dtype(torch.float32)
        assert seen == [], f"{dtype}: PyTorch kernels on the forward path: {seen}"


def test_infer_issues_no_aten_compute_ops(gpu_model):
    """`AcousticModel.infer(steps=4)` with the output length given: the Euler grid lives on the host, the four time embeddings
    are one launch, an Euler step, the duration / pitch / energy algebra, the soft path and the length regulation are libispk
    kernels - a TorchDispatchMode sees only views and allocations."""
    from torch.utils._python_dispatch import TorchDispatchMode
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream")
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func)
            if not name.startswith(harmless):
                seen.append(name)
            return func(*args, **(kwargs or {}))
    inp = synth.make_inputs(3, 40, 96, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 40), 2, dtype=torch.int64, device=DEV)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        try:
            gpu_model.set_compute_dtype(dtype)
            gpu_model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=80)   # staging etc.
            torch.cuda.synchronize()
            del seen[:]
            with Watch():
                mel, ao = gpu_model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=80)
                mel2, _ = gpu_model.infer(text, text_lengths=tl, steps=4, flow_noise=x_t, max_dec_len=128)   # predicted durations
            torch.cuda.synchronize()
        finally:
            gpu_model.set_compute_dtype(torch.float32)
        assert not seen, f"{dtype}: PyTorch compute ops inside infer: {sorted(set(seen))}"
        assert mel.shape == (3, 80, 80) and mel2.shape == (3, 80, 128) and torch.isfinite(mel).all()


def test_headline_batch_infer_bf16_and_split_against_the_oracle(gpu_model, state_dict):
    """`infer(steps=4)` at the benchmarked batch (B=64 x 100 tokens -> 512 frames, duration targets summing to 512) against
    `orc.acoustic_infer`: exact-fp32 and split-fp16 paths to the 1e-4 bar, the bf16 path to its stated bound (four Euler steps
    of a 3-layer AdaLN stack + 12 bf16 layers)."""
    inp = synth.make_inputs(64, 100, 512, variable=True)
    tl = inp["text_len"]
    dur = torch.zeros(64, 100, dtype=torch.int64)
    for b in range(64):
        l, m = int(tl[b]), int(inp["mel_len"][b])
        dur[b, :l] = m // l
        dur[b, : m - (m // l) * l] += 1
    ref_mel, ref_ad = orc.acoustic_infer(state_dict, inp["text"], tl, dur, inp["flow_x0"], 4)
    d = {k: v.to(DEV) for k, v in inp.items()}
    errs = {}
    for name, dtype in (("f32", torch.float32), ("split", torch.float16), ("bf16", torch.bfloat16)):
        try:
            gpu_model.set_compute_dtype(dtype)
            mel, ao = gpu_model.infer(d["text"], text_lengths=d["text_len"], duration_target=dur.to(DEV), steps=4,
                                      flow_noise=d["flow_x0"], max_dec_len=512)
            torch.cuda.synchronize()
        finally:
            gpu_model.set_compute_dtype(torch.float32)
        assert torch.equal(ao.dec_lengths.cpu(), ref_ad.dec_lengths)
        e = (mel[:, :, :ref_mel.shape[2]].cpu().double() - ref_mel.double())
        errs[name] = (e.abs().max().item(), _maxdiff(ao.pitch, ref_ad.pitch),
                      (e.pow(2).mean().sqrt() / ref_mel.double().pow(2).mean().sqrt()).item())
    print("B=64 infer(steps=4) mel L-inf / pitch L-inf / mel relative RMS vs oracle: "
          + ", ".join(f"{k} {v[0]:.2e} / {v[1]:.2e} / {v[2]:.2e}" for k, v in errs.items()))
    assert errs["f32"][0] < MEL_TOL and errs["split"][0] < MEL_TOL
    # bf16: the predicted pitch / energy (four Euler steps through the bf16 predictor) feed the embedding stack, so the
    # operand rounding of the whole adaptor sits in the decoder's INPUT: measured 1.1e-1 L-inf, 1.5e-2 relative RMS
    assert errs["bf16"][0] < INFER_BF16_MEL_TOL and errs["bf16"][2] < 3e-2


def test_graph_refuses_to_replay_after_weights_were_restaged(gpu_model):
    """A captured graph points at the staged weight images; once one is rebuilt (a parameter changed) replaying would read
    freed memory - it raises instead.  The other precision's images live in their own slots and do not invalidate it."""
    from isp_tts_amd.graph import GraphedForward
    inp = {k: v.to(DEV) for k, v in _forward_inputs().items()}
    g = GraphedForward(gpu_model, inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"], inp["energy"],
                       inp["flow_noise"], inp["flow_time"])
    first = g.replay().mel.clone()
    try:
        gpu_model.set_compute_dtype(torch.bfloat16)
        gpu_model(**inp)                       # stages the bf16 images beside the fp32 ones
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    assert torch.equal(g.replay().mel, first)
    w = gpu_model.decoder.layers[0].attention.to_q.weight
    with torch.no_grad():
        w.add_(0.0)                            # bumps the parameter's version: its staged image is stale now
    gpu_model(**inp)
    with pytest.raises(RuntimeError, match="rebuilt after this graph was captured"):
        g.replay()


def test_graph_lanes_reproduce_the_eager_forward(gpu_model):
    """HIP-graph replay on two alternating lanes (isp_tts_amd/graph.py:GraphedForwardLanes, what bench.py times) gives
    bit for bit the eager forward - including the side-stream branches, which become graph edges - and still does after
    new inputs are copied into a lane's static buffers; MAS durations equal the reference golden."""
    from isp_tts_amd.graph import GraphedForwardLanes
    g = golden("forward.npz")
    inp = {k: v.to(DEV) for k, v in _forward_inputs().items()}
    eager = gpu_model(**inp)
    torch.cuda.synchronize()
    lanes = GraphedForwardLanes(gpu_model, inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"],
                                inp["energy"], inp["flow_noise"], inp["flow_time"], lanes=2)
    outs = [lanes.replay() for _ in range(4)]
    torch.cuda.synchronize()
    for out in outs[-2:]:
        assert torch.equal(out.mel, eager.mel)
        assert torch.equal(out.adaptor_output.duration, eager.adaptor_output.duration)
        assert torch.equal(out.adaptor_output.losses["flow_loss"], eager.adaptor_output.losses["flow_loss"])
        assert np.array_equal(out.adaptor_output.dec_lengths.cpu().numpy(), g["dec_lengths"])
    # new inputs into lane 0's static buffers: utterance order swapped -> outputs swapped
    g0, s0 = lanes.lanes[0]
    with torch.cuda.stream(s0):
        swapped = g0(**{k: inp[k].flip(0) for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy", "flow_noise",
                                                     "flow_time")})
    torch.cuda.synchronize()
    assert _maxdiff(swapped.mel.flip(0), eager.mel) < 1e-5


def test_bf16_fused_ffn_matches_two_gemm_path_at_full_size(gpu_model):
    """Decoder stack at the benchmark shape (B=64 x 512 frames -> 32,768 rows, where FeedForward takes the fused
    ispk_ffn_bf16 kernel) against the same stack forced onto the two-GEMM path."""
    x = synth._normal("t/ffnfull/x", (64, 512, 384)).to(DEV)
    lens = torch.full((64,), 512, device=DEV)
    lens[1::3] = 300
    mask = torch.arange(512, device=DEV)[None] < lens[:, None]
    dec = gpu_model.decoder
    try:
        dec.set_compute_dtype(torch.bfloat16)
        fused = dec(x, mask=mask, key_len=lens).out
        dec.seams = replace(plan.SEAMS, fused_min_rows=1 << 30)
        plain = dec(x, mask=mask, key_len=lens).out
    finally:
        dec.seams = None
        dec.set_compute_dtype(torch.float32)
    assert (fused - plain).abs().max() < 4e-2 and (fused - plain).pow(2).mean().sqrt() < 3e-3
    assert (fused * ~mask[..., None]).abs().max() == 0




def test_bf16_layernorm_statistics_handoff_matches_separate_layernorm_at_full_size(gpu_model, monkeypatch):
    """Decoder stack at the benchmark shape with layers 2..6's attention LayerNorm applied inside the q/kv GEMM from the
    previous feed-forward kernel's row statistics (`plan.Seams.stats_layernorm`) against separate LayerNorm launches:
    same fp32 statistics up to the reduction tree, so only 1-ulp bf16 roundings of the normalised operand differ."""
    monkeypatch.setattr(plan, "SEAMS", replace(plan.SEAMS, prenorm_fused=False))   # (without the fused feed-forward kernels)
    x = synth._normal("t/chain/x", (64, 512, 384)).to(DEV)
    lens = torch.full((64,), 512, device=DEV)
    lens[2::5] = 211
    mask = torch.arange(512, device=DEV)[None] < lens[:, None]
    dec = gpu_model.decoder
    try:
        dec.set_compute_dtype(torch.bfloat16)
        dec.seams = replace(plan.SEAMS, stats_layernorm=False)
        plain = dec(x, mask=mask, key_len=lens, out_dtype=torch.bfloat16).out
        dec.seams = replace(plan.SEAMS, stats_layernorm=True)
        handed = dec(x, mask=mask, key_len=lens, out_dtype=torch.bfloat16).out
    finally:
        dec.seams = None                     # back to the default
        dec.set_compute_dtype(torch.float32)
    diff = (handed.float() - plain.float()).abs()
    assert diff.max() < 6e-2 and diff.pow(2).mean().sqrt() < 5e-3
    assert (handed.float() * ~mask[..., None]).abs().max() == 0


def test_bf16_prenorm_feed_forward_matches_separate_layernorm_at_full_size(gpu_model, monkeypatch):
    """Decoder stack at the benchmark shape with feed_forward_norm computed inside the fused feed-forward kernel
    (ispk_attn_out_ffn_bf16, the default) against separate LayerNorm launches (`plan.Seams` with the fused forms off)."""
    x = synth._normal("t/chain/x", (64, 512, 384)).to(DEV)
    lens = torch.full((64,), 512, device=DEV)
    lens[2::5] = 211
    mask = torch.arange(512, device=DEV)[None] < lens[:, None]
    dec = gpu_model.decoder
    try:
        dec.set_compute_dtype(torch.bfloat16)
        fused = dec(x, mask=mask, key_len=lens, out_dtype=torch.bfloat16).out
        monkeypatch.setattr(plan, "SEAMS", replace(plan.SEAMS, prenorm_fused=False, stats_layernorm=False, lnin_self=False))
        plain = dec(x, mask=mask, key_len=lens, out_dtype=torch.bfloat16).out
    finally:
        dec.set_compute_dtype(torch.float32)
    diff = (fused.float() - plain.float()).abs()
    assert diff.max() < 6e-2 and diff.pow(2).mean().sqrt() < 5e-3
    assert (fused.float() * ~mask[..., None]).abs().max() == 0




def test_bf16_encoder_with_layernorms_inside_the_gemms_matches_separate_layernorms(gpu_model, monkeypatch):
    """Encoder-sized stack (two-GEMM feed-forward): attention_norm inside the q/kv GEMM and feed_forward_norm inside the
    first feed-forward GEMM (ispk_gemm_bf16_lnin, statistics by the GEMM's own waves) against separate LayerNorm launches."""
    x = synth._normal("t/lnself/x", (16, 100, 384)).to(DEV)
    lens = torch.full((16,), 100, device=DEV)
    lens[1::3] = 37
    mask = torch.arange(100, device=DEV)[None] < lens[:, None]
    enc = gpu_model.encoder
    try:
        enc.set_compute_dtype(torch.bfloat16)
        # (by default only decoder-sized batches take these paths)
        enc.seams = replace(plan.SEAMS, lnin_self_min_rows=0, fused_min_rows=0, prenorm_fused=False)
        fused = enc(x, mask=mask, key_len=lens).out
        enc.seams = replace(enc.seams, lnin_self=False)
        plain = enc(x, mask=mask, key_len=lens).out
    finally:
        enc.seams = None
        enc.set_compute_dtype(torch.float32)
    diff = (fused - plain).abs()
    assert diff.max() < 6e-2 and diff.pow(2).mean().sqrt() < 5e-3
    assert (fused * ~mask[..., None]).abs().max() == 0


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_final_norm_from_the_split_feed_forward_combine_pass(gpu_model, out_dtype):
    """bf16 path, small batches: the stack's final LayerNorm (transformer.py:205-206, row-masked) comes out of the last layer's
    combine pass (`ispk_ffn_combine_ln_f32`) instead of a launch of its own - same values as the separate LayerNorm on the same
    y (one rounding apart for the bf16 form), masked rows exactly zero; with and without a mask."""
    x = synth._normal("t/finalnorm/x", (16, 100, 384)).to(DEV)
    lens = torch.full((16,), 100, device=DEV)
    lens[2::3] = 41
    mask = torch.arange(100, device=DEV)[None] < lens[:, None]
    enc = gpu_model.encoder
    try:
        enc.set_compute_dtype(torch.bfloat16)
        for m_, l_ in ((mask, lens), (None, None)):
            folded = enc(x, mask=m_, key_len=l_, out_dtype=out_dtype).out
            raw = enc(x, mask=m_, key_len=l_, final_norm=False).out
            sep = runtime.layernorm(raw, enc.norm.weight, enc.norm.bias, row_mask=m_, eps=enc.norm.eps, out_dtype=out_dtype)
            assert folded.dtype == out_dtype and folded.shape == sep.shape
            tol = 2e-5 if out_dtype == torch.float32 else 2.0 ** -7
            assert (folded.float() - sep.float()).abs().max().item() <= tol * max(1.0, sep.float().abs().max().item())
            if m_ is not None:
                assert (folded.float() * ~m_[..., None]).abs().max() == 0
    finally:
        enc.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("bsz,frames", [(64, 512), (32, 512), (12, 400)])
def test_decoder_stack_with_the_layer_halves_in_one_kernel(gpu_model, bsz, frames):
    """bf16 path: to_out + residual + feed_forward_norm + feed-forward + residual (+ the next layer's attention_norm and q/kv
    projection) as ONE kernel per layer (`ispk_attn_out_ffn_bf16` / `_qkv_bf16`, decoder-sized batches; `_split_bf16` from 8,192
    rows) against the same stack with those switches off (separate to_out GEMM, feed-forward kernel and q/kv GEMM): the same
    bf16 products in another fp32 summation order - agreement far inside the bf16 path's own error; masked rows exactly zero."""
    x = synth._normal(f"t/halves/x{bsz}", (bsz, frames, 384)).to(DEV)
    lens = torch.full((bsz,), frames, device=DEV)
    lens[1::3] = frames // 2 + 3
    mask = torch.arange(frames, device=DEV)[None] < lens[:, None]
    dec = gpu_model.decoder
    try:
        dec.set_compute_dtype(torch.bfloat16)
        fused = dec(x, mask=mask, key_len=lens).out
        assert torch.equal(fused, dec(x, mask=mask, key_len=lens).out)
        dec.seams = replace(plan.SEAMS, proj_ffn=False, proj_ffn_split=False, next_qkv=False)
        plain = dec(x, mask=mask, key_len=lens).out
        dec.seams = replace(plan.SEAMS, next_qkv=False)
        no_qkv = dec(x, mask=mask, key_len=lens).out
    finally:
        dec.seams = None
        dec.set_compute_dtype(torch.float32)
    scale = plain.abs().max().item()
    for name, got in (("all in one", fused), ("without the q/kv epilogue", no_qkv)):
        e = (got - plain).abs()
        print(f"decoder stack {bsz} x {frames}, {name}: max |diff| {e.max().item():.3e}, rms {e.pow(2).mean().sqrt().item():.3e} (|out| <= {scale:.1f})")
        assert e.max().item() <= 2e-2 * max(1.0, scale) and e.pow(2).mean().sqrt().item() <= 1e-3 * max(1.0, scale)
        assert (got * ~mask[..., None]).abs().max() == 0


def test_config2_encoder_decoder_scope_fp32(gpu_model, state_dict):
    """BASELINE config 2 (B = 32, TextEncoder + MelDecoder + to_mel on given activations, ragged masks, fp32) against the oracle."""
    bsz = 32                                          # BASELINE config 2's batch
    tok = synth._normal("t/c2/tok", (bsz, 100, 384))
    dec_in = synth._normal("t/c2/dec", (bsz, 512, 384))
    tl, ml = synth.make_lengths(bsz, 100, 512, variable=True, seed=202)
    tl[:4], ml[:4] = torch.tensor([100, 80, 100, 33]), torch.tensor([512, 512, 301, 77])
    em = torch.arange(100)[None] < tl[:, None]
    dm = torch.arange(512)[None] < ml[:, None]
    enc_ref, mel_ref = orc.encoder_decoder(state_dict, tok, em, dec_in, dm)
    enc = gpu_model.encoder(tok.to(DEV), mask=em.to(DEV)).out
    dec = gpu_model.decoder(dec_in.to(DEV), mask=dm.to(DEV)).out
    mel = gpu_model._to_mel(dec, dm.to(DEV))
    assert _maxdiff(enc, enc_ref) < OP_TOL and _maxdiff(mel, mel_ref) < MEL_TOL


def test_rccl_all_gather_of_mel_single_rank():
    """The one collective of the path through RCCL itself (backend "nccl" on ROCm), world_size 1 on this one-GPU box;
    the world_size-2 logic is covered on CPU over gloo (tests/test_host_logic.py)."""
    import os
    import torch.distributed as dist
    from isp_tts_amd import dist as idist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29600 + os.getpid() % 1000))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        mel = synth._normal("t/rccl/mel", (5, 80, 64)).to(DEV)
        lens = torch.tensor([64, 10, 33, 64, 1], device=DEV)
        g, l = idist.all_gather_mel(mel, lens)
        assert g.shape == (1, 5, 80, 64) and torch.equal(g[0], mel) and torch.equal(l[0], lens)
        g2, l2 = idist.all_gather_mel(mel, lens, max_frames=64, max_batch=5)
        assert torch.equal(g2[0], mel)
        full, dec = idist.unshard(g, l, [[3, 0, 4, 1, 2]])
        assert torch.equal(full[3], mel[0]) and int(dec[2]) == 1
        # the overlapped pipeline of bench.py, as a gather to rank 0 (default) and as an all-gather
        for root in (0, None):
            pipe = idist.MelGatherPipeline(5, 80, 64, DEV, root=root)
            src, src_len = torch.empty_like(mel), torch.empty_like(lens)
            for step in range(3):
                src.copy_(mel + step)
                src_len.copy_(lens + step)
                pipe.submit(src, src_len)
                src.fill_(-1.0)
            g3, l3 = pipe.wait()
            assert torch.equal(g3[0], mel + 2) and torch.equal(l3[0], lens + 2)
    finally:
        dist.destroy_process_group()


def test_batch_ingest_feeds_the_forward(gpu_model):
    """Row f4 on the GPU: collator-layout host batches through pinned staging + a copy stream (`ingest.BatchIngest`), the
    next batch's copy queued before the current one is consumed; the forward on the ingested tensors equals the forward on
    directly uploaded ones, for every batch and after slots were reused."""
    from isp_tts_amd import ingest
    ing = ingest.BatchIngest(DEV, max_batch=6, max_text=60, max_mel=200, slots=2)
    host, ref = [], []
    for k, (b, l, m) in enumerate([(6, 60, 200), (4, 37, 150), (5, 60, 96), (6, 44, 200)]):
        inp = synth.make_inputs(b, l, m, variable=True, seed=40 + k)
        host.append((inp, {"text_vector": inp["text"], "text_vector_len": inp["text_len"], "mel": inp["mel"],
                           "mel_len": inp["mel_len"], "pitch": inp["pitch"], "energy": inp["energy"]}))
        d = {k_: v.to(DEV) for k_, v in inp.items()}
        ref.append(gpu_model(d["text"], d["text_len"], d["mel"], d["mel_len"], d["pitch"], d["energy"],
                             flow_noise=d["flow_x0"], flow_time=d["flow_t"]).mel.clone())
    ing.submit(host[0][1])
    for k in range(4):
        if k + 1 < 4:
            ing.submit(host[k + 1][1])             # the next batch's copy is in flight while this one computes
        got = ingest.model_inputs(ing.get())
        assert got["mel"].is_cuda and got["mel"].shape == host[k][0]["mel"].shape
        out = gpu_model(**got, flow_noise=host[k][0]["flow_x0"].to(DEV), flow_time=host[k][0]["flow_t"].to(DEV))
        ing.done()
        assert torch.equal(out.mel, ref[k]), f"batch {k}"


def test_three_graph_forward_equals_the_single_graph(gpu_model):
    """`graph.SegmentedForward` (front / side branch / back as separate HIP graphs on two streams, built from
    `AcousticModel.forward_front / forward_side / forward_back`) returns bit-identical outputs to the one-graph forward and
    to the eager forward, also after the static inputs were replaced."""
    from isp_tts_amd.graph import GraphedForward, SegmentedForward
    inp = {k: v.to(DEV) for k, v in _forward_inputs().items()}
    try:
        gpu_model.set_compute_dtype(torch.bfloat16)
        seg, one = SegmentedForward(gpu_model, **inp), GraphedForward(gpu_model, **inp)
        for trial in range(2):
            a, b = seg.replay(), one.replay()
            torch.cuda.synchronize()
            c = gpu_model(**inp)
            for x, y, z in ((a.mel, b.mel, c.mel), (a.aligner_output.attn_hard, b.aligner_output.attn_hard, c.aligner_output.attn_hard),
                            (a.adaptor_output.log_duration, b.adaptor_output.log_duration, c.adaptor_output.log_duration),
                            (a.adaptor_output.dec_lengths, b.adaptor_output.dec_lengths, c.adaptor_output.dec_lengths),
                            (a.adaptor_output.pitch_target, b.adaptor_output.pitch_target, c.adaptor_output.pitch_target)):
                assert torch.equal(x, y) and torch.equal(x, z)
            inp = {k: (v.flip(0) if v.ndim else v) for k, v in inp.items()}       # other utterance order for the second trial
            seg(**inp)
            one(**inp)
    finally:
        gpu_model.set_compute_dtype(torch.float32)


def test_graph_lifetime_old_graphs_die_outside_captures_and_replays(gpu_model):
    """Holds the fix for the two failures recorded in round 2 (`gpurun_out/r2_b7.err`: abort in ~CUDAGraph, "operation not
    permitted when stream is capturing", raised by the cyclic collector inside `GraphedCall.__init__`; `r2_b6.err`: SIGSEGV in
    `replay`): a graph that has become unreachable only through a reference CYCLE is destroyed by `GraphedCall`'s explicit
    collection BEFORE the next capture starts (the collector is off during the capture), and destroying a graph BETWEEN two
    replays of another one leaves that one intact.  Runs once; nothing here loops to provoke a fault."""
    import gc
    import weakref
    from isp_tts_amd.graph import GraphedForward
    inp = synth.make_inputs(2, 40, 96, variable=True, seed=11)
    d = {k: v.to(DEV) for k, v in inp.items()}
    args = (d["text"], d["text_len"], d["mel"], d["mel_len"], d["pitch"], d["energy"], d["flow_x0"], d["flow_t"])
    g1 = GraphedForward(gpu_model, *args)
    want = g1.replay().mel.clone()
    torch.cuda.synchronize()
    dead = weakref.ref(g1.graph)
    cycle = [g1]
    cycle.append(cycle)                 # unreachable after the del below, but only the CYCLIC collector can free it
    del g1, cycle
    assert dead() is not None           # still alive: reference counting alone did not free it
    g2 = GraphedForward(gpu_model, *args)          # collects the old graph first, captures with the collector off
    assert dead() is None and gc.isenabled()
    assert torch.equal(g2.replay().mel, want)
    # a graph destroyed BETWEEN replays of another graph (device idle at that moment)
    g3 = GraphedForward(gpu_model, *args)
    assert torch.equal(g3.replay().mel, want)
    torch.cuda.synchronize()
    del g3
    gc.collect()
    assert torch.equal(g2.replay().mel, want)
    torch.cuda.synchronize()
