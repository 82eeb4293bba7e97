"""GPU: data.Resampler (ispk_resample_f32) against the float64 direct-sum restatement of tests/frontend_reference.py,
utterance by utterance, for determinism and capture, and in front of the extractor and the training step.

Bound, per output sample (derived, not measured; it holds for any summation order):
    |err| <= (T + C + 2) 2^-24 sum_j |k[p, j]| mean_c |x_c[q o + j]|
the running-error bound of an fp32 dot product of T once-rounded taps (T products and additions, one rounding of each tap)
plus the C - 1 additions and the division of the channel mean and the final rounding."""
import numpy as np
import pytest
import torch

import frontend_reference as fr
from isp_tts_amd import synth
from isp_tts_amd.data import AcousticFeatures, AudioFrontEnd, Resampler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(48000, 22050), (44100, 22050), (24000, 22050), (32000, 22050), (16000, 22050), (8000, 22050), (22050, 24000),
         (22050, 48000), (44100, 48000), (48000, 8000), (22050, 16000), (8000, 44100)]
_KINDS = [(k, a) for a in (0.9, 0.05) for k in synth.CLIP_KINDS]
_TAPS = {}


def taps64(orig, new):
    if (orig, new) not in _TAPS:
        k, o, n, width = fr.dense_taps(orig, new)
        _TAPS[(orig, new)] = (k, o, n, width, fr.taps_per_phase(k, 6, o, n, width))
    return _TAPS[(orig, new)]


def clips(lengths, rate, channels=1, salt=0):
    """One fp32 [C, len] clip per length (kinds and amplitudes cycled; channels are different clips)."""
    out = []
    for i, n in enumerate(lengths):
        ch = []
        for c in range(channels):
            kind, amp = _KINDS[(i * 5 + c * 3 + salt) % len(_KINDS)]
            ch.append(synth.make_clip(kind, n, amp, seed=synth.SEED + c, sample_rate=rate))
        out.append(torch.stack(ch))
    return out


def collate(waves, S=None, pad=float("nan"), strided=False, mono2d=True):
    """[C, len] clips -> (fp32 [B, S] (C = 1, mono2d) or [B, C, S] padded with `pad`, int64 lens).  strided: a row stride of
    S + 3 (no float4 path)."""
    C = waves[0].shape[0]
    S = max(w.shape[1] for w in waves) if S is None else S
    wide = torch.full((len(waves), C, S + (3 if strided else 0)), pad)
    for i, w in enumerate(waves):
        wide[i, :, :w.shape[1]] = w
    a = wide.to(DEV)[:, :, :S]
    if C == 1 and mono2d:
        a = a[:, 0]
    return a, torch.tensor([w.shape[1] for w in waves], dtype=torch.int64)


def check(out, out_len, waves, orig, new, what=""):
    k, o, n, width, T = taps64(orig, new)
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    worst = 0.0
    for b, w in enumerate(waves):
        x = w.numpy()
        C, length = x.shape
        y, mag = fr.resample64(x, k, o, n, width)
        assert out_len[b] == len(y) == fr.out_length(length, o, n), f"{what}[{b}]: out_len {out_len[b]} != {len(y)}"
        assert not out[b, len(y):].any(), f"{what}[{b}]: not zero past out_len"
        err = np.abs(out[b, :len(y)].astype(np.float64) - y)
        bound = (T + C + 2) * 2.0 ** -24 * mag
        bad = ~(err <= bound)                                    # (a NaN is outside the bound)
        ratio = float(np.nan_to_num(err / np.maximum(bound, 1e-300), nan=np.inf).max()) if len(y) else 0.0
        worst = max(worst, ratio)
        assert not bad.any(), f"{what}[{b}] ({C} ch, {length} samples): {int(bad.sum())} samples outside the bound, worst {ratio:.2f} x"
    print(f"{what}: worst error {worst:.3f} of the bound")
    return worst


def edge_lengths(o):
    return [1, o - 1, o, o + 1, 3 * o - 1, 3 * o + 1, 17 * o - 1, 17 * o + 1, 40 * o + o // 2]


@pytest.mark.parametrize("orig,new", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_pairs_match_float64_on_edge_lengths(orig, new):
    """Lengths 1, o - 1, o, o + 1, k o +- 1 in one ragged batch with NaN in the padding."""
    rs = Resampler(orig, new)
    waves = clips([max(1, v) for v in edge_lengths(rs.o)], orig)
    a, lens = collate(waves)
    out, out_len = rs(a, lens.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == (len(waves), rs.out_samples(a.shape[1]))
    check(out, out_len, waves, orig, new, f"{orig}->{new}")


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("orig,new", [(48000, 22050), (22050, 24000)], ids=["48k-22k", "22k-24k"])
def test_batch_sizes(orig, new, B):
    lengths = [int(v) for v in np.random.default_rng(B).integers(1, 30000, B)]
    waves = clips(lengths, orig, salt=B)
    a, lens = collate(waves)
    out, out_len = Resampler(orig, new)(a, lens.to(DEV))
    torch.cuda.synchronize()
    check(out, out_len, waves, orig, new, f"{orig}->{new} B={B}")


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("orig,new", [(44100, 22050), (48000, 22050), (22050, 24000)], ids=["44k-22k", "48k-22k", "22k-24k"])
def test_channels_and_row_stride(orig, new, C, strided):
    """[B, C, S] input (C = 1 as a 3-D tensor too), contiguous and at a row stride of S + 3 (no float4 loads)."""
    rs = Resampler(orig, new)
    waves = clips([5000, 1, 3 * rs.o + 1, 12345], orig, channels=C, salt=C)
    a, lens = collate(waves, strided=strided, mono2d=False)
    assert a.ndim == 3 and a.stride(1) == a.shape[2] + (3 if strided else 0)
    out, out_len = rs(a, lens.to(DEV))
    torch.cuda.synchronize()
    check(out, out_len, waves, orig, new, f"{orig}->{new} C={C} strided={strided}")


@pytest.mark.parametrize("orig", [48000, 44100])
def test_the_longest_utterance(orig):
    """The input length whose output is the recipe's 441,088-sample bound at 22.05 kHz."""
    rs = Resampler(orig, 22050)
    length = 441088 * rs.o // rs.n
    assert rs.out_samples(length) == 441088
    waves = clips([length, 100000 + 27], orig)
    a, lens = collate(waves)
    out, out_len = rs(a, lens.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == (2, 441088) and out_len.tolist()[0] == 441088
    check(out, out_len, waves, orig, 22050, f"{orig} long")


def test_out_of_range_lengths_give_empty_rows():
    """Length 0, above S, and negative: out_len 0 and a zero row; the other rows unaffected."""
    rs = Resampler(48000, 22050)
    w = clips([3000], 48000)[0]
    audio = w.repeat(4, 1).to(DEV)
    lens = torch.tensor([3000, 0, 3001, -5], dtype=torch.int64, device=DEV)
    out, out_len = rs(audio, lens)
    torch.cuda.synchronize()
    assert out_len.tolist() == [fr.out_length(3000, 320, 147), 0, 0, 0]
    assert not out[1:].any()
    check(out[:1], out_len[:1], [w], 48000, 22050, "lens")


def test_repeat_and_graph_replay_are_bit_identical():
    rs = Resampler(48000, 22050)
    waves = clips([int(v) for v in np.random.default_rng(7).integers(1, 30000, 64)], 48000)
    a, lens = collate(waves, pad=0.0)
    ln = lens.to(DEV)
    o1 = [t.clone() for t in rs(a, ln)]
    o2 = rs(a, ln)
    out = rs.empty_outputs(a.shape[0], a.shape[1], DEV)
    rs(a, ln, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rs(a, ln, out=out)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y, z in zip(o1, o2, out):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert o1[0].abs().max() > 0.1


def test_resampler_issues_no_aten_compute_ops():
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.slice", "aten.select", "aten.detach", "aten.alias",
                "aten.is_", "aten.size", "aten.stride", "aten.sym_", "aten.empty_like", "aten.new_empty")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = str(func)
            if not name.startswith(harmless):
                if any(t.is_cuda for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)):
                    seen.append(name)
            return out

    rs = Resampler(44100, 22050)
    front = AudioFrontEnd(rs, AcousticFeatures(sample_rate=22050))
    a, lens = collate(clips([9000, 20000, 1234], 44100, channels=2), pad=0.0)
    mono = a[:, 0]
    ln = lens.to(DEV)
    rs(a, ln)
    front(mono, ln)                           # (the first calls put the tables on the device)
    torch.cuda.synchronize()
    with Spy():
        out, _ = rs(a, ln)
        f = front(mono, ln)
    torch.cuda.synchronize()
    assert seen == [], f"PyTorch kernels inside the front end: {sorted(set(seen))}"
    assert torch.isfinite(out).all() and torch.isfinite(f["mel"]).all()


def test_equal_rates():
    """Mono: the inputs come back untouched (the same tensors).  C > 1: the downmix alone, out_len = audio_len."""
    rs = Resampler(22050, 22050)
    waves = clips([4000, 1, 2999], 22050, channels=2)
    a, lens = collate(waves)
    ln = lens.to(DEV)
    mono = a[:, 0]
    o, ol = rs(mono, ln)
    assert o is mono and ol is ln
    out, out_len = rs(a, ln)
    torch.cuda.synchronize()
    assert out.shape == (3, 4000) and out_len.tolist() == lens.tolist()
    for b, w in enumerate(waves):
        n = w.shape[1]
        want = ((w[0].double() + w[1].double()) / 2).float()           # (one rounding of the sum; halving is exact)
        assert torch.equal(out[b, :n].cpu(), want) and not out[b, n:].any()
    six = clips([1000, 37], 22050, channels=6)
    a6, l6 = collate(six)
    out6, _ = rs(a6, l6.to(DEV))
    for b, w in enumerate(six):
        n = w.shape[1]
        err = (out6[b, :n].cpu().double() - w.double().mean(0)).abs()
        assert (err <= 8 * 2.0 ** -24 * w.double().abs().mean(0)).all()


def test_cpu_tensors_raise():
    from isp_tts_amd import runtime
    with pytest.raises(runtime.IspkError):
        Resampler(48000, 22050)(torch.zeros(1, 100), torch.tensor([100]))


def test_front_end_equals_resampler_then_extractor():
    """AudioFrontEnd == Resampler then AcousticFeatures, bit for bit, on the extractor fixture's clips made at 48 kHz."""
    rs = Resampler(48000, 22050)
    feats = AcousticFeatures(sample_rate=22050, pitch_mean=166.6177, pitch_std=62.5423)
    waves = [synth.make_clip(k, (n * 320) // 147, amp, sample_rate=48000)[None] for k, n, amp in synth.FEATURE_CASES["voices"]]
    a, lens = collate(waves)
    ln = lens.to(DEV)
    audio, audio_len = rs(a, ln)
    want = feats(audio, audio_len)
    got = AudioFrontEnd(rs, feats)(a, ln)
    torch.cuda.synchronize()
    assert torch.equal(got["audio_resampled"], audio) and torch.equal(got["audio_resampled_len"], audio_len)
    for k in ("mel", "mel_len", "pitch", "energy"):
        assert torch.equal(got[k], want[k]), k
    assert int(want["mel_len"].min()) > 10 and torch.isfinite(want["mel"]).all()


# ------------------------------------------------------------------------------------------------------- training from audio
def _model(sd):
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    m = AcousticModel.init(AcousticDims().model_config())
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def test_graphed_step_from_48k_audio_matches_the_step_from_resampled_audio():
    """GraphedTrainStep(features=AudioFrontEnd(...)) on 48 kHz audio against GraphedTrainStep(features=extractor) on the
    resampler's own output: features, total, losses and norm bit-equal over two replays."""
    from isp_tts_amd import train
    seed = 9
    rs = Resampler(48000, 22050)
    feats = AcousticFeatures(sample_rate=22050, pitch_mean=166.6177, pitch_std=62.5423)
    targets = (("harmonic", 160 * 256 + 100), ("chirp", 118 * 256), ("noise", 98 * 256 + 30))
    waves = [synth.make_clip(k, -(-n * 320 // 147), 0.5, seed, sample_rate=48000)[None] for k, n in targets]
    a, lens = collate(waves, pad=0.0)
    ln = lens.to(DEV)
    audio, audio_len = (t.clone() for t in rs(a, ln))
    f = {k: v.clone() for k, v in feats(audio, audio_len).items()}
    assert f["mel"].shape == (3, 80, 160) and f["mel_len"].tolist() == [160, 118, 98]
    inp = synth.make_inputs(3, 52, 160, variable=True, seed=seed)
    common = {k: inp[k].to(DEV) for k in ("text", "text_len", "flow_x0", "flow_t")}
    sd = synth.make_state_dict()

    def run(front):
        torch.manual_seed(21)
        m = _model(sd)
        o = train.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, grad_clip=1.0)
        if front:
            step = train.GraphedTrainStep(m, o, dict(common, audio=a, audio_len=ln), amp=True, features=AudioFrontEnd(rs, feats))
        else:
            step = train.GraphedTrainStep(m, o, dict(common, audio=audio, audio_len=audio_len), amp=True, features=feats)
        res = []
        for _ in range(2):
            total, losses, norm = step()
            torch.cuda.synchronize()
            res.append([total.clone(), {k: v.clone() for k, v in losses.items()}, norm.clone()])
            for k in ("mel", "mel_len", "pitch", "energy"):
                assert torch.equal(step.features[k], f[k]), k
        step.close()
        return res

    x, y = run(True), run(False)
    for p, q in zip(x, y):
        assert torch.equal(p[0], q[0]) and torch.equal(p[2], q[2])
        assert all(torch.equal(p[1][k], q[1][k]) for k in q[1])
        assert torch.isfinite(p[0])
