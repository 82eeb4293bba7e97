"""GPU: the Griffin-Lim mel inversion (isp_tts_amd.griffinlim.GriffinLim: csrc/griffinlim.hip, ispk_mel_to_linear_f32 and one
launch of ispk_griffinlim_step_f32 per projection) against the float64 reference of tests/griffinlim_reference.py.

Inputs: synth.make_clip at amplitude 0.5, cut to n = 256 T samples, kinds cycled.  Frame counts T: 0, 1, 2, 3, 4 (the envelope's
edge cases: fewer frames than the four that overlap), 15, 16, 17 (the 16-hop tile edge), 32, 33 (two tiles, the third of one
hop), each run alone and inside a ragged batch of at most 5 whose padded T exceeds its longest item (two batches hold the ten),
with padded row strides, NaN past the lengths and a sentinel in `out`.

Bounds: mel -> magnitude max |err| <= 1e-4 x the item's largest magnitude; the initial waveform, one step
and four steps from the same start, and one step on a consistent pair, max |err| <= 1e-4 x the item's peak.  Samples are not
compared after more iterations: two phase-retrieval trajectories in different precisions drift apart (torch's fp32 chain and
float64 on the CPU: 2e-7 of the peak after 1 iteration, 6e-7 after 4, 1.6e-4 by 16 to 32).  A full run of 32 iterations is
held to its spectral convergence || |STFT(x)| - M ||_F / || M ||_F, computed on the host in float64 after 0, 1, 2, 4, 8, 16 and
32 iterations: it never rises, and it is within a relative 1e-3 of the float64 reference's from the same start (the quantity is
0.1 to 0.6, the trajectories differ by up to 1.6e-4 of the peak; a wrong halo frame or envelope moves it by per cents).

Measured on gfx950 (worst over the items alone and in the batches; torch's fp32 chain on the CPU in brackets):
    mel -> magnitude, fp32 and fp16 mel   max |err| / largest magnitude 2.4e-7   (1.4e-7 to 2.2e-7)
    initial waveform                      max |err| / peak 2.7e-7
    one step                              max |err| / peak 4.5e-7                (2e-7)
    four steps                            max |err| / peak 7.6e-7                (6e-7)
    fixed point                           max |err| / peak 3.0e-7                (2.4e-7)
    spectral convergence, 7 counts        relative difference to float64 at most 9.0e-8 harmonic, 4.3e-7 chirp, 1.3e-7 noise (3e-6)
    mel round trip                        ratio after 32 iterations over after 0: harmonic 0.262, noise 0.101 (float64: the same)

Then the mel round trip through the feature extractor, bit identity (ragged batch = alone, padding contents, lengths out of
range, repeated calls, graph replay, seeds, an all-zero magnitude), the whole text -> PCM16 chain as one graph, score_infer, and
the absence of ATen compute."""
import numpy as np
import pytest
import torch

import griffinlim_reference as gr
from isp_tts_amd import graph, runtime, synth
from isp_tts_amd.data import AcousticFeatures
from isp_tts_amd.griffinlim import GriffinLim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_REL = 1e-4
TS = runtime.GRIFFINLIM_TILE_SAMPLES
FRAMES = (0, 1, 2, 3, 4, 15, 16, 17, 32, 33)
BATCHES = {"a": (0, 2, 16, 33, 4), "b": (1, 3, 15, 17, 32)}
assert sorted(t for b in BATCHES.values() for t in b) == sorted(FRAMES) and TS == 16 * 256
FULL_RUN = (("harmonic", 8192), ("chirp", 12032), ("noise", 4096))
COUNTS = (0, 1, 2, 4, 8, 16, 32)
SENTINEL = 7.0
KINDS = ("harmonic", "noise", "chirp", "edge_hi", "edge_lo")

@pytest.fixture(scope="module")
def gl():
    return GriffinLim(n_iter=32, seed=0).to(DEV)


@pytest.fixture(scope="module")
def fb():
    return AcousticFeatures().fb.double().numpy()


@pytest.fixture(scope="module")
def items(fb):
    """T -> the item's clip (float64 holding fp32 values), its float64 magnitude rounded to fp32, its log-mel rounded to fp32
    and the float64 waveforms after 0, 1 and 4 iterations from the hashed phase of seed 0; made once, never changed."""
    cache = {}

    def get(T):
        if T not in cache:
            x = synth.make_clip(KINDS[T % len(KINDS)], 256 * T, 0.5).double().numpy()
            M = np.abs(gr.stft(x)).astype(np.float32).astype(np.float64)
            mel = gr.log_mel(x, fb).astype(np.float32)
            cache[T] = dict(x=x, M=M, mel=mel, ref=gr.griffinlim(M, 4, seed=0, keep=(0, 1, 4)))
        return cache[T]
    return get


def _mag_batch(mags, Tp, fill=float("nan")):
    """[T_b, 513] float64 each -> fp32 [B, Tp, 513] on the GPU with a padded leading stride; `fill` in every frame past T_b."""
    B = len(mags)
    flat = torch.full((B, Tp * 513 + 7), fill, dtype=torch.float32)
    m = flat.as_strided((B, Tp, 513), (Tp * 513 + 7, 513, 1))
    for b, M in enumerate(mags):
        m[b, :M.shape[0]] = torch.from_numpy(M).float()
    return flat.to(DEV).as_strided((B, Tp, 513), (Tp * 513 + 7, 513, 1))


def _audio_batch(xs, Tp, fill=float("nan")):
    a = torch.full((len(xs), 256 * Tp + 5), fill, dtype=torch.float32)
    for b, x in enumerate(xs):
        a[b, :len(x)] = torch.from_numpy(x).float()
    return a.to(DEV)[:, :256 * Tp]


def _iterate(gl, mags, lens, Tp, n_iter, seed=0, init=None, fill=float("nan"), use_len=True):
    """-> (audio [B, 256 Tp] on the CPU, audio_len [B]); checks the sentinel columns and the returned objects."""
    B, S = len(mags), 256 * Tp
    o = torch.full((B, S + 3), SENTINEL, device=DEV)
    ol = torch.full((B,), -5, dtype=torch.int64, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV) if use_len else None
    a = None if init is None else _audio_batch(init, Tp, fill)
    got, got_len = gl.from_magnitude(_mag_batch(mags, Tp, fill), ln, init=a, n_iter=n_iter, seed=seed, out=(o[:, :S], ol))
    torch.cuda.synchronize()
    assert got.data_ptr() == o.data_ptr() and got_len is ol
    assert (o[:, S:] == SENTINEL).all(), "columns past 256 T were written"
    return o[:, :S].cpu(), ol.cpu()


def _check_item(got, want, what):
    """One utterance's row against float64: the bound below n, exact zeros from n on."""
    n = len(want)
    assert (got[n:] == 0).all(), f"{what}: non-zero samples at or past n"
    if n == 0:
        return 0.0
    peak = float(np.abs(want).max())
    err = float(np.abs(got[:n].double().numpy() - want).max())
    print(f"{what}: max|err| / peak = {err / peak:.2e}")
    assert err <= FP32_REL * peak, f"{what}: max |err| {err:.3e} > 1e-4 x peak {peak:.3e}"
    return err / peak


# ----------------------------------------------------------------------------------------------------- mel -> magnitude
def _mel_batch(mels, Tp, dtype):
    m = torch.full((len(mels), 80, Tp + 3), float("nan"), dtype=dtype)
    for b, mel in enumerate(mels):
        m[b, :, :mel.shape[1]] = torch.from_numpy(mel).to(dtype)
    return m.to(DEV)[:, :, :Tp]


def _check_magnitude(gl, fb, mels, Tp, dtype, what):
    P = gr.pinv(fb)
    ln = torch.tensor([m.shape[1] for m in mels], dtype=torch.int64, device=DEV)
    out = _mag_batch([np.zeros((0, 513))] * len(mels), Tp, fill=SENTINEL)
    got = gl.magnitude(_mel_batch(mels, Tp, dtype), ln, out=out)
    torch.cuda.synchronize()
    assert got is out
    got = got.cpu()
    worst = 0.0
    for b, mel in enumerate(mels):
        T = mel.shape[1]
        assert (got[b, T:] == SENTINEL).all(), f"{what}[{b}]: a frame at or past mel_len was written"
        if T == 0:
            continue
        want = gr.mel_to_linear(torch.from_numpy(mel).to(dtype).double().numpy(), P)     # the values the kernel read
        top = float(want.max())
        err = float(np.abs(got[b, :T].double().numpy() - want).max())
        assert top > 1.0 and (want == 0).any() and (got[b, :T] >= 0).all()             # the clamp acts
        print(f"mel -> magnitude {what}[{b}] T={T}: max|err| / largest = {err / top:.2e}")
        assert err <= FP32_REL * top, f"{what}[{b}]: max |err| {err:.3e} > 1e-4 x {top:.3e}"
        worst = max(worst, err / top)
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_mel_to_magnitude_against_float64(gl, fb, items, dtype):
    assert runtime.lib().ispk_griffinlim_tile_samples() == TS
    for T in FRAMES:
        _check_magnitude(gl, fb, [items(T)["mel"]], T + 1, dtype, f"alone {T}")
    for name, lens in BATCHES.items():
        _check_magnitude(gl, fb, [items(T)["mel"] for T in lens], max(lens) + 2, dtype, f"batch {name}")
    # without lengths every frame is written
    mel = items(17)["mel"]
    got = gl.magnitude(torch.from_numpy(mel).to(dtype).to(DEV)[None])
    want = gr.mel_to_linear(torch.from_numpy(mel).to(dtype).double().numpy(), gr.pinv(fb))
    assert got.shape == (1, 17, 513) and float(np.abs(got[0].cpu().double().numpy() - want).max()) <= FP32_REL * want.max()


# --------------------------------------------------------------------------------------- init, one step, four steps
@pytest.mark.parametrize("T", FRAMES)
def test_init_one_and_four_steps_alone(gl, items, T):
    it = items(T)
    for n_iter in (0, 1, 4):
        got, alen = _iterate(gl, [it["M"]], [T], T + 1, n_iter)
        assert alen.tolist() == [256 * T]
        if T:
            assert float(np.abs(it["ref"][n_iter]).max()) > 1e-3
        _check_item(got[0], it["ref"][n_iter], f"alone T={T}, {n_iter} iterations")


@pytest.mark.parametrize("name", list(BATCHES))
def test_init_one_and_four_steps_ragged(gl, items, name):
    lens = BATCHES[name]
    Tp = max(lens) + 2
    for n_iter in (0, 1, 4):
        got, alen = _iterate(gl, [items(T)["M"] for T in lens], lens, Tp, n_iter)
        assert alen.tolist() == [256 * T for T in lens]
        for b, T in enumerate(lens):
            _check_item(got[b], items(T)["ref"][n_iter], f"batch {name} T={T}, {n_iter} iterations")


def test_without_lengths(gl, items):
    """mel_len None: every utterance has all T frames (T = 17: two tiles, the second of one hop)."""
    a, b = items(17), items(17)
    got, alen = _iterate(gl, [a["M"], b["M"]], None, 17, 1, use_len=False)
    assert alen.tolist() == [256 * 17] * 2 and torch.equal(got[0], got[1])
    _check_item(got[0], a["ref"][1], "no lengths")


def test_fixed_point(gl, items):
    """init = a clip, the magnitude its own (float64, rounded to fp32): one step returns the clip."""
    for lens in BATCHES.values():
        xs = [items(T)["x"] for T in lens]
        got, _ = _iterate(gl, [items(T)["M"] for T in lens], lens, max(lens) + 1, 1, init=xs)
        for b, T in enumerate(lens):
            _check_item(got[b], xs[b], f"fixed point T={T}")


# --------------------------------------------------------------------------------------------------------------- full run
@pytest.mark.parametrize("kind,n", FULL_RUN)
def test_full_run_spectral_convergence(gl, kind, n):
    T = n // 256
    x = synth.make_clip(kind, n, 0.5).double().numpy()
    M = np.abs(gr.stft(x)).astype(np.float32).astype(np.float64)
    ref = gr.griffinlim(M, 32, seed=0, keep=COUNTS)
    waves, prev = {}, None
    for a, c in zip((0,) + COUNTS, COUNTS):                        # 0, then each count from the one before it through init=
        got, _ = _iterate(gl, [M], [T], T, c - a, init=prev)
        waves[c] = got[0].double().numpy()
        prev = [waves[c]]
    straight, _ = _iterate(gl, [M], [T], T, 32)
    assert np.array_equal(straight[0].double().numpy(), waves[32]), "32 iterations in one call differ from the chained calls"
    sc = [gr.spectral_convergence(waves[c], M) for c in COUNTS]
    sc_ref = [gr.spectral_convergence(ref[c], M) for c in COUNTS]
    rel = [abs(a - b) / b for a, b in zip(sc, sc_ref)]
    print(f"{kind}: spectral convergence {['%.5f' % v for v in sc]}, float64 {['%.5f' % v for v in sc_ref]}, "
          f"relative difference {['%.1e' % v for v in rel]}")
    assert all(b <= a for a, b in zip(sc, sc[1:])), f"{kind}: the spectral convergence rises: {sc}"
    assert max(rel) <= 1e-3, f"{kind}: spectral convergence {sc} against float64 {sc_ref}"
    assert sc[0] > 0.3 and sc[-1] < 0.25


@pytest.mark.parametrize("kind,n", [("harmonic", 8192), ("noise", 4096)])
def test_mel_round_trip(kind, n):
    """clip -> AcousticFeatures -> GriffinLim -> AcousticFeatures: 32 iterations halve the mean |log-mel difference| of the
    initial waveform at least (the float64 reference: 0.26 and 0.10 of it)."""
    feats = AcousticFeatures(pitch=False, energy=False)
    gl = GriffinLim.from_features(feats, n_iter=32, seed=0).to(DEV)
    audio = synth.make_clip(kind, n, 0.5).to(DEV)[None]
    alen = torch.tensor([n], dtype=torch.int64, device=DEV)
    f = feats(audio, alen)
    mel, mel_len = f["mel"].clone(), f["mel_len"].clone()
    assert mel_len.tolist() == [n // 256]
    diff = {}
    for n_iter in (0, 32):
        wav, wlen = gl.from_magnitude(gl.magnitude(mel, mel_len), mel_len, n_iter=n_iter)
        assert wlen.tolist() == [n] and wav.shape == (1, n)
        diff[n_iter] = float((feats(wav, wlen)["mel"] - mel).abs().mean())
    whole, _ = gl(mel, mel_len)                                     # the module's call: its own n_iter
    assert torch.equal(whole, wav)
    print(f"{kind}: mean |log-mel difference| {diff[0]:.4f} -> {diff[32]:.4f}, ratio {diff[32] / diff[0]:.3f}")
    assert diff[32] < 0.5 * diff[0]


# ----------------------------------------------------------------------------------------------------------- bit identity
def test_ragged_batch_equals_alone_and_ignores_padding(gl, items):
    lens = BATCHES["a"]
    Tp = max(lens) + 2
    mags = [items(T)["M"] for T in lens]
    base, base_len = _iterate(gl, mags, lens, Tp, 3)
    for b, T in enumerate(lens):                                           # an utterance alone, in a shorter row
        alone, _ = _iterate(gl, [mags[b]], [T], T + 1, 3)
        assert torch.equal(alone[0, :256 * T], base[b, :256 * T]), f"T={T}: the batch changed an utterance's bits"
    for fill in (0.0, 1e30):                                               # base ran with NaN past the lengths
        assert torch.equal(_iterate(gl, mags, lens, Tp, 3, fill=fill)[0], base), f"fill {fill}"
    assert torch.equal(_iterate(gl, mags, lens, Tp, 3)[0], base)           # a second call
    other, _ = _iterate(gl, mags, lens, Tp, 3, seed=1)                     # another seed: another start
    assert not torch.equal(other, base) and torch.equal(_iterate(gl, mags, lens, Tp, 3, seed=1)[0], other)
    # an init waveform with NaN / 1e30 past the lengths
    xs = [items(T)["x"] * 0.5 for T in lens]
    from_init, _ = _iterate(gl, mags, lens, Tp, 2, init=xs)
    assert torch.equal(_iterate(gl, mags, lens, Tp, 2, init=xs, fill=1e30)[0], from_init)
    assert torch.isfinite(from_init).all() and not torch.equal(from_init, _iterate(gl, mags, lens, Tp, 2)[0])
    # device lengths outside [0, T]: zero rows, length 0
    wide = [np.concatenate([M, np.ones((Tp - M.shape[0], 513))]) for M in mags]      # finite everywhere
    bad, bad_len = _iterate(gl, wide, (-1, 2, Tp + 1, 33, 4), Tp, 3)
    assert bad_len.tolist() == [0, 512, 0, 256 * 33, 1024]
    assert (bad[0] == 0).all() and (bad[2] == 0).all()
    for b in (1, 3, 4):
        assert torch.equal(bad[b], base[b])


def test_zero_magnitude_gives_exact_zeros(gl, items):
    lens = (4, 17, 1)
    zeros = [np.zeros((T, 513)) for T in lens]
    got, _ = _iterate(gl, zeros, lens, 18, 2)
    assert (got == 0).all()
    got, _ = _iterate(gl, zeros, lens, 18, 1, init=[items(T)["x"] for T in lens])      # a loud waveform projected onto silence
    assert (got == 0).all()
    # silence projected onto a magnitude: |X| = 0 everywhere, so Y = M with phase 0; finite, and not silence
    got, _ = _iterate(gl, [items(T)["M"] for T in lens], lens, 18, 1, init=[np.zeros(256 * T) for T in lens])
    want = gr.step(np.zeros(256 * 17), items(17)["M"])
    _check_item(got[1], want, "silence onto a magnitude")


def test_module_call_and_graph_replay(gl, fb, items):
    from isp_tts_amd.data import to_pcm16
    lens = (4, 17, 0, 33)
    Tp = 34
    mel = _mel_batch([items(T)["mel"] for T in lens], Tp, torch.float32)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV)
    eager, alen = gl(mel, ln)
    again, _ = gl(mel, ln)
    torch.cuda.synchronize()
    assert eager.shape == (4, 256 * Tp) and alen.tolist() == [256 * T for T in lens] and torch.equal(eager, again)
    for b, T in enumerate(lens):
        assert (eager[b, 256 * T:] == 0).all() and (T == 0 or float(eager[b].abs().max()) > 0.02)
    inp, out = mel.clone(), gl.empty_outputs(4, Tp, DEV)
    g = graph.GraphedCall(lambda: gl(inp, ln, out=out))
    out[0].zero_()
    out[1].zero_()
    got, got_len = g.replay()
    torch.cuda.synchronize()
    assert got.data_ptr() == out[0].data_ptr() and torch.equal(out[0], eager) and torch.equal(out[1], alen)
    for parity in (3, 4):                                                  # the last iterate lands in `out` for odd and even counts
        o = gl.empty_outputs(4, Tp, DEV)
        mag = gl.magnitude(mel, ln)
        gp = graph.GraphedCall(lambda: gl.from_magnitude(mag, ln, n_iter=parity, out=o))
        want, _ = gl.from_magnitude(mag, ln, n_iter=parity)
        o[0].zero_()
        gp.replay()
        torch.cuda.synchronize()
        assert torch.equal(o[0], want), f"n_iter={parity}"
    # a length outside [0, T] is a zero row here and counts as 0 in the stage that follows
    bad = torch.tensor([Tp + 1, 17, -3, 33], dtype=torch.int64, device=DEV)
    z, zl = gl(torch.nan_to_num(mel), bad)
    pcm = to_pcm16(z, zl)
    torch.cuda.synchronize()
    assert zl.tolist() == [0, 256 * 17, 0, 256 * 33] and (z[0] == 0).all() and (z[2] == 0).all() and torch.equal(z[1], eager[1])
    assert (pcm[0] == 0).all() and (pcm[2] == 0).all()
    # zero frames, and refusals
    e, el = gl(mel[:, :, :0], None)
    assert e.shape == (4, 0) and el.tolist() == [0] * 4
    with pytest.raises(ValueError, match="nothing to iterate"):
        gl.from_magnitude(gl.magnitude(mel, ln), ln, init=eager, n_iter=0)
    with pytest.raises(runtime.IspkError, match="may not be audio"):
        gl.from_magnitude(gl.magnitude(mel, ln), ln, init=eager, n_iter=1, out=(eager, alen))
    with pytest.raises(ValueError, match="mel"):
        gl(mel[:, :79], ln)


# ----------------------------------------------------------------------------------------------------------- whole chain
def _acoustic_model():
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    return model.to(DEV).requires_grad_(False)


@pytest.fixture(scope="module")
def model():
    return _acoustic_model()


def test_text_to_pcm16_as_one_graph(model):
    """text -> mel -> GriffinLim -> conditioned -> PCM16, captured as one HIP graph: the replay equals the eager chain."""
    from isp_tts_amd.data import AudioConditioner, to_pcm16
    gl = GriffinLim(n_iter=4).to(DEV)
    cond = AudioConditioner(22050)
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 30), 2, dtype=torch.int64, device=DEV)
    wav = gl.empty_outputs(3, 64, DEV)
    out = cond.empty_outputs(3, wav[0].shape[1], DEV)
    pcm = torch.empty(wav[0].shape, dtype=torch.int16, device=DEV)

    def chain():
        mel, ao = model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=64)
        audio, audio_len = gl(mel, ao.dec_lengths, out=wav)
        r = cond(audio, audio_len, out=out)
        return to_pcm16(r["audio"], r["audio_len"], out=pcm), r

    chain()
    torch.cuda.synchronize()
    eager_pcm, eager_wav, eager = pcm.clone(), wav[0].clone(), {k: v.clone() for k, v in out.items()}
    assert (wav[1] >= 256).all() and float(wav[0].abs().max()) > 0
    g = graph.GraphedCall(chain)
    pcm.zero_()
    wav[0].zero_()
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pcm, eager_pcm) and torch.equal(wav[0], eager_wav)
    for k in eager:
        assert eager[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k
    assert (out["audio_len"] > 0).all() and pcm.abs().max() > 100


def test_score_infer_with_griffinlim(model):
    from isp_tts_amd.acoustic.evaluator import SynthesisEvaluator
    gl = GriffinLim(n_iter=4).to(DEV)
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    pitch_hz = synth.make_stats_case("voices")["pitch"][:3, :64] * (torch.arange(64)[None] < inp["mel_len"][:, None])
    inputs = {"text": inp["text"].to(DEV), "text_len": inp["text_len"].to(DEV), "mel": inp["mel"].to(DEV),
              "mel_len": inp["mel_len"].to(DEV), "pitch_hz": pitch_hz.to(DEV)}
    kw = {"duration_target": torch.full((3, 30), 2, dtype=torch.int64, device=DEV), "steps": 4,
          "flow_noise": inp["flow_x0"].to(DEV), "max_dec_len": 64}
    ev, feats = SynthesisEvaluator(), AcousticFeatures(pitch_mean=0.0, pitch_std=1.0)
    got = ev.score_infer(model, inputs, vocoder=gl, features=feats, **kw)
    mel, ao = model.infer(inputs["text"], text_lengths=inputs["text_len"], **kw)
    audio, alen = gl(mel, ao.dec_lengths)
    want = ev(mel, ao.dec_lengths, inputs["mel"], inputs["mel_len"], feats(audio, alen)["pitch"], inputs["pitch_hz"])
    torch.cuda.synchronize()
    assert list(got) == list(want) and len(got) == 4
    assert all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in got)
    for k in ("metrics/mcd_dtw_13", "metrics/vuv_error", "metrics/length_ratio"):
        assert bool(torch.isfinite(got[k])), got
    # f0_rmse_cents is NaN by definition when no aligned pair of frames is voiced on both sides (tests/dtw_reference.py), which
    # the mel of a model with random weights may give; it is never infinite
    assert not bool(torch.isinf(got["metrics/f0_rmse_cents"])), got


def test_griffinlim_issues_no_aten_compute_ops(gl, items):
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

    mel = _mel_batch([items(17)["mel"], items(4)["mel"]], 18, torch.float32)
    ln = torch.tensor([17, 4], dtype=torch.int64, device=DEV)
    out, init = gl.empty_outputs(2, 18, DEV), torch.zeros((2, 256 * 18), device=DEV)
    gl(mel, ln)
    torch.cuda.synchronize()
    with Watch():
        gl(mel, ln)
        gl(mel, ln, out=out)
        gl(mel, None)
        mag = gl.magnitude(mel, ln)
        gl.from_magnitude(mag, ln, n_iter=0)
        gl.from_magnitude(mag, ln, init=init, n_iter=3, seed=5, out=out)
    torch.cuda.synchronize()
    assert not seen, f"PyTorch compute ops inside GriffinLim: {sorted(set(seen))}"
