"""GPU: the vocoder denoiser (isp_tts_amd.denoiser.Denoiser: csrc/denoise.hip, one launch of ispk_denoise_f32) against the
float64 reference of tests/denoiser_reference.py.

Inputs: a 220 Hz sine of amplitude 0.3 plus Gaussian noise of 0.1, another seed per item.  Lengths (TS = the kernel's tile,
runtime.DENOISE_TILE_SAMPLES): 0, 1, 512, 513, 514, 767, 768, 769, 1024, 1025, TS - 1, TS, TS + 1, 2 TS + 255, each run alone
and inside a ragged batch of at most 5 utterances whose S exceeds its longest (three batches hold the fourteen lengths), with
padded row strides and a sentinel in `out`; one more batch runs without audio_len.

Bound: max |out - ref64| <= 1e-4 x max |ref64| per utterance.  The bias is the per-bin median of the
float64 |X| over an item's frames at strength 1, so about half the bins are clamped to zero and half are shrunk: the share of
zeroed bins is asserted to lie in [0.3, 0.7] for every item of at least 3 frames.  A ragged batch has one bias (the kernel takes
one per call): that of its longest item.  Measured on gfx950: worst max |err| / peak 3.5e-7 alone and 2.7e-7 in the batches
(torch's own fp32 chain on the same inputs, on the CPU: 1.6e-7 to 3.6e-7).

Then the strength's two ends, per-item strengths, bit identity (ragged batch = alone, padding contents, lengths out of range,
repeated calls, graph replay), Denoiser.from_vocoder, the whole text -> PCM16 chain as one graph, score_infer, and the absence
of ATen compute."""
import numpy as np
import pytest
import torch

import denoiser_reference as dr
from isp_tts_amd import graph, runtime, synth
from isp_tts_amd.denoiser import Denoiser, denoise_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_REL = 1e-4
TS = runtime.DENOISE_TILE_SAMPLES
LENGTHS = (0, 1, 512, 513, 514, 767, 768, 769, 1024, 1025, TS - 1, TS, TS + 1, 2 * TS + 255)
# the fourteen lengths in batches of at most 5, short and long ones mixed, tile edges next to copies
BATCHES = {"a": (0, 513, 1024, TS - 1, 769), "b": (1, 514, 1025, TS, 767), "c": (512, 768, TS + 1, 2 * TS + 255)}
assert sorted(n for b in BATCHES.values() for n in b) == sorted(LENGTHS)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def tables():
    return denoise_tables().to(DEV)


@pytest.fixture(scope="module")
def signals():
    """length -> the item's waveform (float64 holding fp32 values), its float64 spectrum's per-bin median, made once."""
    cache = {}

    def get(n):
        if n not in cache:
            x = dr.make_signal(n, seed=1000 + n)
            cache[n] = (x, np.median(np.abs(dr.stft(x)), axis=0) if n >= dr.MIN_SAMPLES else np.ones(dr.K))
        return cache[n]
    return get


def _run(tables, xs, lens, bias, strength, S, use_len=True, pad_in=5, pad_out=3, fill=float("nan")):
    """xs: the utterances (float64); the rest of each row is `fill`, never to be read.  -> out [B, S] on the CPU."""
    B = len(xs)
    a = torch.full((B, S + pad_in), fill, dtype=torch.float32)
    for b, x in enumerate(xs):
        a[b, :len(x)] = torch.from_numpy(x).float()
    o = torch.full((B, S + pad_out), SENTINEL, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV) if use_len else None
    st = strength.to(DEV) if isinstance(strength, torch.Tensor) else strength
    got = runtime.denoise(a.to(DEV)[:, :S], ln, tables, torch.from_numpy(np.asarray(bias, dtype=np.float32)).to(DEV), st,
                          out=o[:, :S])
    torch.cuda.synchronize()
    assert got.data_ptr() == o.data_ptr()
    assert (o[:, S:] == SENTINEL).all(), "columns past S were written"
    return o[:, :S].cpu()


def _check_item(got, x, want, what):
    """One utterance's row against float64: the bound below n, exact zeros from n on, a bit copy below 513 samples."""
    n = len(x)
    assert (got[n:] == 0).all(), f"{what}: non-zero samples at or past n"
    if n < dr.MIN_SAMPLES:
        assert torch.equal(got[:n], torch.from_numpy(x).float()), f"{what}: a short utterance is copied bit for bit"
        return 0.0
    peak = float(np.abs(want).max())
    err = float(np.abs(got[:n].double().numpy() - want).max())
    assert err <= FP32_REL * peak, f"{what}: max |err| {err:.3e} > 1e-4 x peak {peak:.3e}"
    return err / peak


def _torch_fp32_chain(x, bias, strength):
    w = torch.hann_window(1024, periodic=True)
    X = torch.stft(torch.from_numpy(x).float(), 1024, hop_length=256, win_length=1024, window=w, center=True,
                   pad_mode="reflect", return_complex=True)
    mag = X.abs()
    t = strength * torch.from_numpy(bias).float()[:, None]
    Y = torch.where(mag > 0, X * torch.clamp(1 - t / mag, min=0), torch.zeros_like(X))
    return torch.istft(Y, 1024, hop_length=256, win_length=1024, window=w, center=True, length=len(x)).double().numpy()


# ------------------------------------------------------------------------------------------------ kernel against float64
@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_against_float64_alone(tables, signals, n):
    assert runtime.lib().ispk_denoise_tile_samples() == TS and TS % 256 == 0
    x, bias = signals(n)
    S = n + 37
    got = _run(tables, [x], [n], bias, 1.0, S)
    want = dr.denoise(x, bias, 1.0)
    if n >= dr.MIN_SAMPLES:
        share = dr.zeroed_share(x, bias, 1.0)
        assert 0.3 <= share <= 0.7, f"n={n}: the reference zeroes {share:.2f} of the bins"
        assert float(np.abs(want - x).max()) > 1e-2                      # and the denoised waveform is not the input
    rel = _check_item(got[0], x, want, f"n={n}")
    if n >= dr.MIN_SAMPLES:
        tch = float(np.abs(_torch_fp32_chain(x, bias, 1.0) - want).max() / np.abs(want).max())
        print(f"denoise alone n={n}: max|err| / peak = {rel:.2e} (torch fp32 chain on the CPU: {tch:.2e}), zeroed share {share:.2f}")


@pytest.mark.parametrize("name", list(BATCHES))
def test_kernel_against_float64_ragged(tables, signals, name):
    lens = BATCHES[name]
    S = max(lens) + 129
    xs = [signals(n)[0] for n in lens]
    bias = signals(max(lens))[1]                                          # one bias per call: the longest item's median
    got = _run(tables, xs, lens, bias, 1.0, S)
    worst = 0.0
    for b, n in enumerate(lens):
        if n >= dr.MIN_SAMPLES:
            share = dr.zeroed_share(xs[b], bias, 1.0)
            assert 0.3 <= share <= 0.7, f"batch {name} n={n}: the reference zeroes {share:.2f} of the bins"
        worst = max(worst, _check_item(got[b], xs[b], dr.denoise(xs[b], bias, 1.0), f"batch {name} n={n}"))
    print(f"denoise batch {name} {lens}: worst max|err| / peak = {worst:.2e}")


def test_kernel_without_lengths(tables, signals):
    """audio_len NULL: every utterance has all S samples (S = TS + 1: two tiles, the second of one sample)."""
    S = TS + 1
    xs = [signals(S)[0], dr.make_signal(S, seed=5)]
    bias = signals(S)[1]
    got = _run(tables, xs, None, bias, 1.0, S, use_len=False)
    for b in range(2):
        _check_item(got[b], xs[b], dr.denoise(xs[b], bias, 1.0), f"no lengths, item {b}")


# --------------------------------------------------------------------------------------------------------------- strength
def test_strength_zero_and_saturation(tables, signals):
    lens = (512, 513, 769, TS + 1, 100)
    S = TS + 200
    xs = [signals(n)[0] if n in LENGTHS else dr.make_signal(n, seed=n) for n in lens]
    bias = signals(TS + 1)[1]
    back = _run(tables, xs, lens, bias, 0.0, S)                            # strength 0: a round trip
    for b, n in enumerate(lens):
        rel = _check_item(back[b], xs[b], xs[b], f"strength 0 n={n}")
        assert rel <= FP32_REL
    # a strength above every |X| / bias: Y = 0 exactly, so every sample below n is 0.0; below 513 samples still a copy
    top = max(float((np.abs(dr.stft(x)) / bias[None, :]).max()) for x in xs if len(x) >= dr.MIN_SAMPLES)
    assert float(bias.min()) > 0
    gone = _run(tables, xs, lens, bias, 2.0 * top, S)
    for b, n in enumerate(lens):
        if n >= dr.MIN_SAMPLES:
            assert (gone[b] == 0).all(), f"n={n}: samples survive a strength above every |X| / bias"
        else:
            assert torch.equal(gone[b, :n], torch.from_numpy(xs[b]).float()) and (gone[b, n:] == 0).all()


def test_per_item_strength(tables, signals):
    lens = (769, TS + 1, 513, 300)
    S = TS + 64
    xs = [signals(n)[0] if n in LENGTHS else dr.make_signal(n, seed=n) for n in lens]
    bias = signals(TS + 1)[1]
    scalar = _run(tables, xs, lens, bias, 0.75, S)
    same = _run(tables, xs, lens, bias, torch.full((4,), 0.75), S)
    assert torch.equal(scalar, same)                                       # equal per-item values: the scalar call's bits
    values = [0.0, 0.5, 1.0, 2.0]
    mixed = _run(tables, xs, lens, bias, torch.tensor(values), S)
    for b, n in enumerate(lens):
        alone = _run(tables, [xs[b]], [n], bias, values[b], n + 11)
        assert torch.equal(mixed[b, :n], alone[0, :n]) and (mixed[b, n:] == 0).all(), f"item {b}"
    assert not torch.equal(mixed[1], scalar[1])
    ref = dr.denoise_batch(np.stack([np.pad(x, (0, S - len(x))) for x in xs]), lens, bias, values)
    for b, n in enumerate(lens):
        _check_item(mixed[b], xs[b], ref[b, :n], f"per-item strength, item {b}")


# ----------------------------------------------------------------------------------------------------------- bit identity
def test_ragged_batch_equals_alone_and_ignores_padding(tables, signals):
    lens = (513, TS, 2 * TS + 255, 1, 1025)
    S = 2 * TS + 300
    xs = [signals(n)[0] for n in lens]
    bias = signals(2 * TS + 255)[1]
    base = _run(tables, xs, lens, bias, 1.0, S)
    for b, n in enumerate(lens):                                           # an utterance alone, in a shorter row
        alone = _run(tables, [xs[b]], [n], bias, 1.0, n + 3)
        assert torch.equal(alone[0, :n], base[b, :n]), f"n={n}: the batch changed an utterance's bits"
    for fill in (0.0, 1e30):                                               # base ran with NaN past the lengths
        assert torch.equal(_run(tables, xs, lens, bias, 1.0, S, fill=fill), base), f"fill {fill}"
    assert torch.equal(_run(tables, xs, lens, bias, 1.0, S), base)         # a second call
    # device lengths outside [0, S]: zero rows; downstream stages count the passed-through length as 0 too
    bad = _run(tables, xs, (-1, TS, S + 1, 1, 1025), bias, 1.0, S)
    assert (bad[0] == 0).all() and (bad[2] == 0).all() and torch.equal(bad[1], base[1]) and torch.equal(bad[4], base[4])


def test_module_call_and_graph_replay(signals):
    from isp_tts_amd.data import to_pcm16
    lens = (769, TS + 1, 0, 513)
    S = TS + 40
    bias = signals(TS + 1)[1]
    den = Denoiser(torch.from_numpy(bias), strength=1.0).to(DEV)
    a = torch.zeros((4, S))
    for b, n in enumerate(lens):
        a[b, :n] = torch.from_numpy(signals(n)[0]).float()
    a, ln = a.to(DEV), torch.tensor(lens, dtype=torch.int64, device=DEV)
    eager, alen = den(a, ln)
    assert alen is ln                                                      # audio_len is passed through
    again, _ = den(a, ln)
    assert torch.equal(eager, again)
    want = dr.denoise_batch(a.cpu().numpy(), lens, bias, 1.0)
    for b, n in enumerate(lens):
        _check_item(eager[b].cpu(), signals(n)[0], want[b, :n], f"module, item {b}")
    half, _ = den(a, ln, strength=0.5)
    assert not torch.equal(half, eager)
    inp, out = a.clone(), torch.empty_like(a)
    g = graph.GraphedCall(lambda: den(inp, ln, out=out))
    out.zero_()
    got, _ = g.replay()
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, eager)
    inp.copy_(a.flip(0))                                                   # new inputs through the captured call
    want2, _ = den(a.flip(0).contiguous(), ln)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2) and not torch.equal(want2, eager)
    # a length outside [0, S] is a zero row here and counts as 0 in the stage that follows
    bad = torch.tensor([S + 1, TS + 1, -3, 513], dtype=torch.int64, device=DEV)
    z, zl = den(a, bad)
    pcm = to_pcm16(z, zl)
    torch.cuda.synchronize()
    assert (z[0] == 0).all() and (z[2] == 0).all() and torch.equal(z[1], eager[1]) and (pcm[0] == 0).all() and (pcm[2] == 0).all()


# ---------------------------------------------------------------------------------------------------------- from_vocoder
def _vocoder(kind):
    if kind == "hifigan":
        from isp_tts_amd.hifigan import HifiGan
        cfg = synth.HIFIGAN_DIMS["odd"]
        return HifiGan.from_state_dict(synth.make_hifigan_state_dict(cfg), cfg).to(DEV).eval()
    from isp_tts_amd.bigvgan import BigVGan
    cfg = synth.BIGVGAN_DIMS["odd"]
    return BigVGan.from_state_dict(synth.make_bigvgan_state_dict(cfg), cfg).to(DEV).eval()


@pytest.mark.parametrize("kind", ["hifigan", "bigvgan"])
def test_from_vocoder(kind):
    voc = _vocoder(kind)
    hop = voc.hop_length
    frames = max(88, -(-2048 // hop))
    for mode in ("zeros", "normal"):
        den = Denoiser.from_vocoder(voc, mode=mode, seed=3, strength=0.25)
        assert den.bias_spec.is_cuda and den.bias_spec.shape == (1, 513, 1) and den.strength == 0.25
        mel = torch.zeros((1, voc.n_mels, frames)) if mode == "zeros" else \
            torch.randn((1, voc.n_mels, frames), generator=torch.Generator().manual_seed(3))
        audio, alen = voc(mel.to(DEV))
        n = int(alen[0])
        assert n == frames * hop >= 2048
        want = np.abs(dr.stft(audio[0, :n].cpu().double().numpy())[0])     # frame 0 of the vocoder's own output, float64
        got = den.bias_spec.flatten().cpu().double().numpy()
        assert float(want.max()) > 0
        assert (np.abs(got - want) <= 2.0 ** -24 * want * (1 + 1e-9) + 1e-30).all(), f"{kind} {mode}: more than one fp32 rounding"
        if mode == "normal":
            again = Denoiser.from_vocoder(voc, mode="normal", seed=3)
            other = Denoiser.from_vocoder(voc, mode="normal", seed=4)
            assert torch.equal(again.bias_spec, den.bias_spec) and not torch.equal(other.bias_spec, den.bias_spec)
    den = Denoiser.from_vocoder(voc, frames=frames + 2)
    assert den.strength == 0.01
    with pytest.raises(ValueError, match="at least 513"):
        Denoiser.from_vocoder(voc, frames=2)


# ----------------------------------------------------------------------------------------------------------- whole chain
def _acoustic_model():
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    return model.to(DEV).requires_grad_(False)


@pytest.fixture(scope="module")
def chain_parts():
    from isp_tts_amd.hifigan import HifiGan
    cfg = synth.HIFIGAN_DIMS["v3"]
    voc = HifiGan.from_state_dict(synth.make_hifigan_state_dict(cfg), cfg).to(DEV).eval()
    return _acoustic_model(), voc, Denoiser.from_vocoder(voc, strength=0.5)


def test_text_to_pcm16_as_one_graph(chain_parts):
    """text -> mel -> HiFi-GAN -> Denoiser -> conditioned -> PCM16, captured as one HIP graph: the replay equals the eager chain."""
    from isp_tts_amd.data import AudioConditioner, to_pcm16
    model, voc, den = chain_parts
    cond = AudioConditioner(22050)
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 30), 2, dtype=torch.int64, device=DEV)
    wav = voc.empty_outputs(3, 64, DEV)
    clean = torch.empty_like(wav[0])
    out = cond.empty_outputs(3, wav[0].shape[1], DEV)
    pcm = torch.empty(wav[0].shape, dtype=torch.int16, device=DEV)

    def chain():
        mel, ao = model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=64)
        audio, audio_len = voc(mel, ao.dec_lengths, out=wav)
        audio, audio_len = den(audio, audio_len, out=clean)
        r = cond(audio, audio_len, out=out)
        return to_pcm16(r["audio"], r["audio_len"], out=pcm), r

    chain()
    torch.cuda.synchronize()
    eager_pcm, eager = pcm.clone(), {k: v.clone() for k, v in out.items()}
    assert not torch.equal(clean, wav[0]) and (wav[1] >= 513).all()        # the denoiser did something
    g = graph.GraphedCall(chain)
    pcm.zero_()
    clean.zero_()
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pcm, eager_pcm)
    for k in eager:
        assert eager[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k
    assert (out["audio_len"] > 0).all() and pcm.abs().max() > 100


def test_score_infer_with_a_denoiser(chain_parts):
    from isp_tts_amd.acoustic.evaluator import SynthesisEvaluator
    from isp_tts_amd.data import AcousticFeatures
    model, voc, den = chain_parts
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    pitch_hz = synth.make_stats_case("voices")["pitch"][:3, :64] * (torch.arange(64)[None] < inp["mel_len"][:, None])
    inputs = {"text": inp["text"].to(DEV), "text_len": inp["text_len"].to(DEV), "mel": inp["mel"].to(DEV),
              "mel_len": inp["mel_len"].to(DEV), "pitch_hz": pitch_hz.to(DEV)}
    kw = {"duration_target": torch.full((3, 30), 2, dtype=torch.int64, device=DEV), "steps": 4,
          "flow_noise": inp["flow_x0"].to(DEV), "max_dec_len": 64}
    ev, feats = SynthesisEvaluator(), AcousticFeatures(pitch_mean=0.0, pitch_std=1.0)
    got = ev.score_infer(model, inputs, vocoder=voc, features=feats, denoiser=den, **kw)
    # the same scores from the pieces, the denoiser between the vocoder and the feature extractor
    mel, ao = model.infer(inputs["text"], text_lengths=inputs["text_len"], **kw)
    audio, alen = den(*voc(mel, ao.dec_lengths))
    want = ev(mel, ao.dec_lengths, inputs["mel"], inputs["mel_len"], feats(audio, alen)["pitch"], inputs["pitch_hz"])
    torch.cuda.synchronize()
    assert list(got) == list(want) and len(got) == 4
    assert all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in got)
    for k in ("metrics/mcd_dtw_13", "metrics/vuv_error", "metrics/length_ratio"):
        assert bool(torch.isfinite(got[k])), got
    # f0_rmse_cents is NaN by definition when no aligned pair of frames is voiced on both sides (tests/dtw_reference.py), which a
    # generator with random weights may give (test_gpu_hifigan.test_score_infer_with_hifigan); it is never infinite
    assert not bool(torch.isinf(got["metrics/f0_rmse_cents"])), got
    # denoiser=None: what score_infer returned before it took one - the scores of the vocoder's own waveform
    none = ev.score_infer(model, inputs, vocoder=voc, features=feats, denoiser=None, **kw)
    default = ev.score_infer(model, inputs, vocoder=voc, features=feats, **kw)
    raw_audio, raw_len = voc(mel, ao.dec_lengths)
    pieces = ev(mel, ao.dec_lengths, inputs["mel"], inputs["mel_len"], feats(raw_audio, raw_len)["pitch"], inputs["pitch_hz"])
    torch.cuda.synchronize()
    for k in pieces:
        assert torch.equal(none[k].view(torch.int32), pieces[k].view(torch.int32)), k
        assert torch.equal(default[k].view(torch.int32), pieces[k].view(torch.int32)), k


def test_denoiser_issues_no_aten_compute_ops(signals):
    from torch.utils._python_dispatch import TorchDispatchMode
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream")
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not str(func).startswith(harmless):
                seen.append(str(func))
            return func(*args, **(kwargs or {}))

    den = Denoiser(torch.from_numpy(signals(1025)[1])).to(DEV)
    a = torch.from_numpy(np.stack([np.pad(signals(n)[0], (0, 1100 - n)) for n in (1025, 769)])).float().to(DEV)
    ln = torch.tensor([1025, 769], dtype=torch.int64, device=DEV)
    per_item, out = torch.tensor([0.5, 1.0], device=DEV), torch.empty_like(a)
    den(a, ln)
    torch.cuda.synchronize()
    with Watch():
        den(a, ln)
        den(a, ln, strength=0.3)
        den(a, ln, strength=per_item, out=out)
        den(a, None)
    torch.cuda.synchronize()
    assert not seen, f"PyTorch compute ops inside Denoiser: {sorted(set(seen))}"
