"""GPU: data.AudioConditioner (ispk_audio_measure_f64 + ispk_audio_apply_f32) and data.to_pcm16 (ispk_pcm16) against the
float64 restatement of tests/conditioning_reference.py, utterance by utterance; batch independence, determinism, capture, and
the conditioner inside AudioFrontEnd and behind the vocoder.

Gate and trim decisions are compared exactly.  That is meaningful only for inputs that keep a margin: `reference()` asserts,
for EVERY item of every case, that each 400 ms block is at least MARGIN_DB from both gates and each trim frame at least
MARGIN_DB from the trim threshold (the float64 sums of kernel and restatement differ by summation order, some 1e-12 dB)."""
import functools
import math

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import conditioning_reference as cr
from isp_tts_amd import graph, synth
from isp_tts_amd.data import AcousticFeatures, AudioConditioner, AudioFrontEnd, Resampler, to_pcm16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN_DB = 1e-6
# |L_gpu - L_ref| in dB.  Measured on the MI355X over every case of this file: at most 7.417e-10 dB (the 19,200-sample 42 Hz
# tone at 48 kHz, one block; 2.4e-11 dB on the other 48 kHz clips, 1.7e-11 dB at 22.05 kHz, 1.1e-12 dB at 16 kHz); the bound
# is 4 x that (summation order differs between kernel and restatement).  A float64 kernel: orders below the 4.4e-5 dB of a
# sequential fp32 evaluation, and far inside the 1e-3 dB no bound here may exceed.
LOUDNESS_BOUND_DB = 4 * 7.417e-10
PEAK_LIMIT = 10 ** (-1 / 20)


def speech_like():
    return np.concatenate([np.zeros(7000, np.float32), synth.make_clip("harmonic", 30000, 0.7).numpy(),
                           synth.make_clip("noise", 15000, 1e-4).numpy(), synth.make_clip("chirp", 40000, 0.3).numpy(),
                           np.zeros(9000, np.float32)])


def peaky():
    """Quiet noise with one full-scale click: the gain to -23 LUFS would clip, so the peak cap decides."""
    x = synth.make_clip("noise", 40000, 0.01).numpy().copy()
    x[12345] = 0.9
    return x


@functools.lru_cache(maxsize=None)
def clips(rate):
    mk = lambda kind, n, amp: synth.make_clip(kind, n, amp, sample_rate=rate).numpy()
    if rate == 22050:
        return (mk("harmonic", 131072, 0.5), mk("chirp", 100000, 0.3), mk("noise", 65537, 0.2), mk("edge_lo", 44100, 0.9),
                mk("harmonic", 60000, 1e-3), mk("silence", 30000, 0.5), mk("harmonic", 8819, 0.5), mk("harmonic", 8820, 0.5),
                np.zeros(0, np.float32), speech_like(), peaky())
    if rate == 16000:
        return (mk("harmonic", 50001, 0.4), mk("chirp", 44100, 0.6), mk("noise", 6399, 0.3), mk("noise", 6400, 0.3))
    return (mk("chirp", 131072, 0.5), mk("harmonic", 70000, 0.05), mk("edge_lo", 19200, 0.7), mk("edge_lo", 19199, 0.7))


CONFIGS = {"default": {}, "no_trim": dict(top_db=None), "const_ref_pad": dict(top_db=40.0, ref=1.0, pad_frames=2),
           "shift_only": dict(target_lufs=None), "loud_target": dict(target_lufs=-14.0, top_db=30.0, pad_frames=1)}


@functools.lru_cache(maxsize=None)
def reference(rate, config):
    """The float64 results of every clip of `rate` under CONFIGS[config], with the margin asserted for every item."""
    kw = CONFIGS[config]
    out = []
    for i, x in enumerate(clips(rate)):
        gate, frame = cr.margins_db(x, rate, kw.get("top_db", 60.0), kw.get("ref", "max"))
        assert gate >= MARGIN_DB and frame >= MARGIN_DB, f"{rate} Hz clip {i} ({config}): gate margin {gate:.2e} dB, frame margin {frame:.2e} dB"
        out.append(cr.condition(x, rate, **dict(dict(target_lufs=-23.0, peak_limit=PEAK_LIMIT), **kw)))
    return out


def collate(waves, S=None, pad=float("nan"), strided=False):
    """fp32 [B, S] padded with `pad` (never read), int64 lens; strided: a row stride of S + 3 (no float4 loads)."""
    S = max(len(w) for w in waves) if S is None else S
    wide = torch.full((len(waves), S + (3 if strided else 0)), pad)
    for i, w in enumerate(waves):
        wide[i, :len(w)] = torch.from_numpy(np.ascontiguousarray(w))
    return wide.to(DEV)[:, :S], torch.tensor([len(w) for w in waves], dtype=torch.int64, device=DEV)


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def check(r, waves, refs, rate, target, what):
    """Everything the conditioner returned for a batch against the per-item references; returns the largest loudness error."""
    torch.cuda.synchronize()
    g = {k: v.cpu().numpy() for k, v in r.items()}
    worst = 0.0
    for b, (x, ref) in enumerate(zip(waves, refs)):
        tag = f"{what}[{b}] ({len(x)} samples)"
        start, end = ref["start"], ref["end"]
        assert g["bounds"][b].tolist() == [start, end], f"{tag}: bounds {g['bounds'][b].tolist()} != {[start, end]}"
        assert g["audio_len"][b] == end - start
        assert g["peak"][b].tobytes() == ref["peak"].tobytes(), f"{tag}: peak {g['peak'][b]!r} != {ref['peak']!r}"
        L = float(g["loudness"][b])
        if ref["loudness"] == -math.inf:
            assert L == -math.inf, f"{tag}: loudness {L} for no gated block"
            assert g["gain"][b] == 1.0
        else:
            err = abs(L - ref["loudness"])
            print(f"{tag}: L = {L:.6f} LKFS, |L_gpu - L_ref| = {err:.3e} dB, {int(ref['both'].sum())} of {len(ref['z'])} blocks")
            worst = max(worst, err)
            assert err <= LOUDNESS_BOUND_DB, f"{tag}: loudness {L} vs {ref['loudness']}"
        if target is None:
            assert g["gain"][b] == 1.0
        assert ulps(g["gain"][b], ref["gain"]) <= 2, f"{tag}: gain {g['gain'][b]!r} vs {ref['gain']!r}"
        want = g["gain"][b] * x[start:end]                          # one fp32 product per sample
        assert g["audio"][b, :end - start].tobytes() == want.astype(np.float32).tobytes(), f"{tag}: out != gain_gpu * x[start + i]"
        assert not g["audio"][b, end - start:].any(), f"{tag}: not zero past out_len"
    print(f"{what}: largest |L_gpu - L_ref| = {worst:.3e} dB")
    return worst


@pytest.mark.parametrize("config", list(CONFIGS))
def test_22050_batch_against_float64(config):
    """Harmonic, chirp, noise, edge_lo, the -67 LKFS clip, silence, 8,819 / 8,820 samples, length 0, the speech-like item
    and the peak-capped one in one ragged batch with NaN in the padding."""
    waves, refs = clips(22050), reference(22050, config)
    if config == "default":
        quiet, none, one, sp, pk = refs[4], refs[6], refs[7], refs[9], refs[10]
        assert -67.5 < quiet["loudness"] < -66.5 and quiet["absolute"].all()
        assert len(none["z"]) == 0 and len(one["z"]) == 1 and refs[5]["loudness"] == -math.inf and refs[8]["end"] == 0
        assert (sp["start"], sp["end"]) == (6144, 92928)
        assert pk["gain"] == np.float32(PEAK_LIMIT / float(pk["peak"])) and pk["peak"] == np.float32(0.9)      # the cap engaged
        assert 10.0 ** ((-23.0 - pk["loudness"]) / 20.0) > 2.0 * float(pk["gain"])
    if config == "no_trim":
        sp = refs[9]
        assert (len(sp["z"]), int(sp["absolute"].sum()), int(sp["both"].sum())) == (42, 39, 37) and abs(sp["loudness"] + 12.9732) < 1e-4
    cond = AudioConditioner(22050, **CONFIGS[config])
    a, ln = collate(waves)
    check(cond(a, ln), waves, refs, 22050, cond.target_lufs, f"22050 {config}")


@pytest.mark.parametrize("rate", [16000, 48000])
def test_other_rates(rate):
    """16 kHz and 48 kHz, with the lengths one below and at one block (6,399 / 6,400 and 19,199 / 19,200 samples)."""
    waves, refs = clips(rate), reference(rate, "no_trim")
    assert len(refs[2]["z"]) + len(refs[3]["z"]) == 1
    a, ln = collate(waves)
    check(AudioConditioner(rate, top_db=None)(a, ln), waves, refs, rate, -23.0, f"{rate} no_trim")
    check(AudioConditioner(rate)(a, ln), waves, reference(rate, "default"), rate, -23.0, f"{rate} default")


def test_unaligned_row_stride_and_base():
    """A row stride of S + 3 and a base 4 bytes off a 16-byte boundary: the scalar-load paths of all three kernels."""
    waves, refs = clips(22050), reference(22050, "default")
    cond = AudioConditioner(22050)
    a, ln = collate(waves, strided=True)
    assert a.stride(0) % 4 != 0
    r = cond(a, ln)
    check(r, waves, refs, 22050, -23.0, "strided")
    sub = [w[1:] for w in waves[:4]]
    a2, ln2 = collate(waves[:4], pad=0.0)
    shifted = a2[:, 1:]
    assert shifted.data_ptr() % 16 == 4
    r2 = cond(shifted, ln2 - 1)
    torch.cuda.synchronize()
    for b, x in enumerate(sub):
        gate, frame = cr.margins_db(x, 22050)
        assert gate >= MARGIN_DB and frame >= MARGIN_DB
        ref = cr.condition(x, 22050)
        assert r2["bounds"][b].tolist() == [ref["start"], ref["end"]] and abs(float(r2["loudness"][b]) - ref["loudness"]) <= LOUDNESS_BOUND_DB
    pcm = to_pcm16(a, ln)
    torch.cuda.synchronize()
    for b, x in enumerate(waves):
        assert np.array_equal(pcm[b].cpu().numpy(), cr.pcm16(np.pad(x, (0, a.shape[1] - len(x))), len(x)))


def test_out_of_range_lengths_count_as_zero():
    cond = AudioConditioner(22050)
    x = clips(22050)[3][:20000]
    a = torch.from_numpy(x).repeat(4, 1).to(DEV)
    r = cond(a, torch.tensor([20000, 0, 20001, -5], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    ref = cr.condition(x, 22050)
    assert r["bounds"].tolist() == [[ref["start"], ref["end"]], [0, 0], [0, 0], [0, 0]]
    assert r["loudness"][1:].tolist() == [-math.inf] * 3 and r["gain"][1:].tolist() == [1.0] * 3 and not r["audio"][1:].any()
    assert abs(float(r["loudness"][0]) - ref["loudness"]) <= LOUDNESS_BOUND_DB


def test_batch_independence_and_repeats():
    """Item b alone (B = 1) and inside a batch of 64 (other neighbours, another grid): every output bit-identical; a second
    call repeats the first bit for bit."""
    base = clips(22050)
    order = [(7 * i + 3) % len(base) for i in range(64)]
    a, ln = collate([base[i] for i in order], pad=0.0)
    cond = AudioConditioner(22050)
    big = {k: v.clone() for k, v in cond(a, ln).items()}
    again = cond(a, ln)
    torch.cuda.synchronize()
    for k in big:
        assert big[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    seen = set()
    for b, i in enumerate(order):
        if i in seen:
            continue
        seen.add(i)
        one = cond(a[b:b + 1], ln[b:b + 1])
        torch.cuda.synchronize()
        for k in big:
            assert one[k][0].cpu().numpy().tobytes() == big[k][b].cpu().numpy().tobytes(), f"item {b} (clip {i}): {k} differs between B = 1 and B = 64"
    assert len(seen) == len(base)


# ------------------------------------------------------------------------------------------------------------------ PCM16
def test_pcm16_without_dither_is_bit_exact():
    """+-1.0, beyond full scale, the half-way values (ties to even), values around the last code, and NaN / junk past audio_len."""
    half = [(k + 0.5) / 32768.0 for k in range(-5, 5)] + [32766.5 / 32768.0, 32767.5 / 32768.0, -32767.5 / 32768.0]
    vals = [1.0, -1.0, 2.0, -2.0, 0.0, -0.0, 0.99999, -0.99999, 1e-9, 32767.0 / 32768.0, 0.25 / 32768.0, 0.75 / 32768.0] + half
    row = np.array(vals + [float("nan"), 0.7, -0.7], dtype=np.float32)
    n = len(vals)
    x = np.stack([row, np.roll(row, 3), synth.make_clip("harmonic", len(row), 1.2).numpy()])
    lens = [n, len(row), 17]
    x[1, np.isnan(x[1])] = 0.3
    got = to_pcm16(torch.from_numpy(x).to(DEV), torch.tensor(lens, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert got.dtype == torch.int16
    for b in range(3):
        assert np.array_equal(got[b].cpu().numpy(), cr.pcm16(x[b], lens[b])), b
    q = got[0].cpu().numpy()
    assert q[:4].tolist() == [32767, -32768, 32767, -32768] and not q[n:].any()
    assert q[12:22].tolist() == [-4, -4, -2, -2, 0, 0, 2, 2, 4, 4]                    # half to even
    waves = clips(22050)
    a, ln = collate(waves)
    pcm = to_pcm16(a, ln)
    torch.cuda.synchronize()
    for b, w in enumerate(waves):
        assert np.array_equal(pcm[b].cpu().numpy(), cr.pcm16(np.pad(w, (0, a.shape[1] - len(w))), len(w)))


def test_pcm16_dither():
    """TPDF of +-1 LSB over 2^20 samples of a slow ramp: a pure function of (seed, b, i), |q - 32768 x| < 1.5, the error mean
    within 0.01 LSB of 0 and its variance within 2 % of 1/4 LSB^2 (1/6 of the dither + 1/12 of the rounding)."""
    n = 1 << 20
    ramp = np.linspace(-0.45, 0.45, n).astype(np.float32)
    x = torch.from_numpy(np.stack([ramp, ramp[::-1].copy()])).to(DEV)
    ln = torch.tensor([n, n - 1000], dtype=torch.int64, device=DEV)
    q1 = to_pcm16(x, ln, dither=True, seed=5)
    q2 = to_pcm16(x, ln, dither=True, seed=5)
    q3 = to_pcm16(x, ln, dither=True, seed=6)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2) and not torch.equal(q1, q3)
    q = q1.cpu().numpy()
    assert not q[1, n - 1000:].any()
    for b, (row, m) in enumerate(((ramp, n), (ramp[::-1], n - 1000))):
        assert np.array_equal(q[b], cr.pcm16(row, m, True, 5, b)), f"row {b}: not the (seed, b, i) hash of the definition"
        err = q[b, :m].astype(np.float64) - 32768.0 * row[:m].astype(np.float64)
        assert np.abs(err).max() < 1.5
        print(f"dither row {b}: error mean {err.mean():+.5f} LSB, variance {err.var():.5f} LSB^2")
        assert abs(err.mean()) <= 0.01 and abs(err.var() - 0.25) <= 0.02 * 0.25
    assert not np.array_equal(q[0, :4096], q[1, :4096][::-1])                          # rows draw different sequences
    plain = to_pcm16(x, ln).cpu().numpy()
    e0 = plain[0].astype(np.float64) - 32768.0 * ramp.astype(np.float64)
    assert np.abs(e0).max() <= 0.5


# ------------------------------------------------------------------------------------------- in the pipeline, and captured
class _Spy(TorchDispatchMode):
    HARMLESS = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.slice", "aten.select", "aten.detach", "aten.alias",
                "aten.is_", "aten.size", "aten.stride", "aten.sym_", "aten.empty_like", "aten.new_empty")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_flatten
        out = func(*args, **(kwargs or {}))
        if not str(func).startswith(self.HARMLESS):
            if any(t.is_cuda for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)):
                self.seen.append(str(func))
        return out


def _front_inputs():
    waves = [synth.make_clip(k, n, amp, sample_rate=48000).numpy() for k, n, amp in
             (("harmonic", 70000, 0.4), ("chirp", 52345, 0.2), ("noise", 30000, 0.05))]
    waves[0][:9000] = 0.0
    waves[1][-7000:] = 0.0
    return collate(waves, pad=0.0)


def test_front_end_with_conditioner_issues_no_aten_ops_and_captures():
    rs, feats = Resampler(48000, 22050), AcousticFeatures(sample_rate=22050, pitch_mean=166.6177, pitch_std=62.5423)
    cond = AudioConditioner(22050)
    front = AudioFrontEnd(rs, feats, conditioner=cond)
    a, ln = _front_inputs()
    out = front.empty_outputs(a.shape[0], a.shape[1], DEV)
    front(a, ln, out=out)                                           # (the first call puts the tables on the device)
    torch.cuda.synchronize()
    spy = _Spy()
    with spy:
        front(a, ln, out=out)
        pcm = to_pcm16(out["audio_conditioned"], out["audio_conditioned_len"])
    torch.cuda.synchronize()
    assert spy.seen == [], f"PyTorch kernels inside the conditioned front end: {sorted(set(spy.seen))}"
    # resample, condition, extract: each stage on the previous one's output
    audio, audio_len = rs(a, ln)
    c = cond(audio, audio_len)
    want = feats(c["audio"], c["audio_len"])
    torch.cuda.synchronize()
    assert torch.equal(out["audio_resampled"], audio) and torch.equal(out["audio_conditioned"], c["audio"])
    assert torch.equal(out["audio_conditioned_len"], c["audio_len"]) and torch.equal(out["bounds"], c["bounds"])
    for k in ("mel", "mel_len", "pitch", "energy"):
        assert torch.equal(out[k], want[k]), k
    assert (out["bounds"][:, 0] > 0).any() and (out["audio_conditioned_len"] < out["audio_resampled_len"]).any()
    assert torch.isfinite(out["loudness"]).all() and pcm.abs().max() > 1000
    eager = {k: v.clone() for k, v in out.items()}
    g = graph.GraphedCall(lambda: front(a, ln, out=out))
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert eager[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k


def test_front_end_without_conditioner_is_unchanged():
    rs, feats = Resampler(48000, 22050), AcousticFeatures(sample_rate=22050, pitch_mean=166.6177, pitch_std=62.5423)
    a, ln = _front_inputs()
    got = AudioFrontEnd(rs, feats)(a, ln)
    audio, audio_len = rs(a, ln)
    want = feats(audio, audio_len)
    torch.cuda.synchronize()
    assert set(got) == {"mel", "mel_len", "pitch", "energy", "audio_resampled", "audio_resampled_len"}
    assert torch.equal(got["audio_resampled"], audio) and torch.equal(got["audio_resampled_len"], audio_len)
    for k in ("mel", "mel_len", "pitch", "energy"):
        assert torch.equal(got[k], want[k]), k


def test_text_to_pcm16_as_one_graph():
    """text -> mel -> waveform -> conditioned -> PCM16 (dithered), captured as one HIP graph: the replay equals the eager chain."""
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    from isp_tts_amd.vocoder import Vocoder
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    model = model.to(DEV).requires_grad_(False)
    voc = Vocoder.from_state_dict(synth.make_vocoder_state_dict(synth.VOCODER_DIMS["official"])).to(DEV).eval()
    cond = AudioConditioner(22050)
    inp = synth.make_inputs(3, 40, 96, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 40), 2, dtype=torch.int64, device=DEV)
    wav = voc.empty_outputs(3, 80, DEV)
    out = cond.empty_outputs(3, wav[0].shape[1], DEV)
    pcm = torch.empty(wav[0].shape, dtype=torch.int16, device=DEV)

    def chain():
        mel, ao = model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=80)
        audio, audio_len = voc(mel, ao.dec_lengths, out=wav)
        r = cond(audio, audio_len, out=out)
        return to_pcm16(r["audio"], r["audio_len"], dither=True, seed=3, out=pcm), r

    chain()
    torch.cuda.synchronize()
    eager_pcm, eager = pcm.clone(), {k: v.clone() for k, v in out.items()}
    g = graph.GraphedCall(chain)
    pcm.zero_()
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pcm, eager_pcm)
    for k in eager:
        assert eager[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k
    assert (out["audio_len"] > 0).all() and pcm.abs().max() > 100
