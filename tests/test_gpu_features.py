"""GPU: the feature extractor (data.AcousticFeatures -> ispk_audio_features_f32) against a float64 restatement of the
reference's providers kept here (an explicit DFT, direct-sum torch-yin), against the reference's own providers and collator
(tests/golden/features.npz, tools/make_feature_goldens.py), for determinism and capture, and inside the training step.

Bounds: log-mel within 1e-4 where the float64 mel is >= 1e-2 of its frame's largest, linear mel within
2e-6 of the frame's largest elsewhere (both clamped at 1e-5); energy within 1e-5 relative; the YIN lag equal on every frame
whose float64 decision is not fragile (a comparison at or before it within 1e-4 of the threshold, or a slope within 1e-6 of
0), fragile frames at most 2 % of a case; pitch bit-equal wherever the lag is; mel_len exact; zeros past it."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

from isp_tts_amd import config, synth
from isp_tts_amd.data import AcousticFeatures, collate_audio, pitch_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, TAU_MIN, TAU_MAX, THR, MEAN, STD = 22050, 27, 525, 0.15, 166.6177, 62.5423


def extractor():
    return AcousticFeatures(sample_rate=SR, pitch_mean=MEAN, pitch_std=STD)


# ---------------------------------------------------------------------------------------------------------------- float64
def _basis():
    n = np.arange(1024)[:, None]
    k = np.arange(513)[None, :]
    a = 2 * np.pi * ((n * k) % 1024) / 1024
    return np.cos(a), np.sin(a)


_BASIS = None


def reference64(wave: np.ndarray, fb: np.ndarray):
    """One utterance, float64: linear mel [80, T], energy [T], cmdf slices [P, 497] (the YIN frames), T, P."""
    global _BASIS
    if _BASIS is None:
        _BASIS = _basis()
    x = wave.astype(np.float64)
    xp = np.pad(x, (384, 384))
    T = (len(xp) - 1024) // 256 + 1
    idx = np.arange(T)[:, None] * 256 + np.arange(1024)[None, :]
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)               # periodic Hann
    fr = xp[idx] * win
    re, im = fr @ _BASIS[0], -(fr @ _BASIS[1])
    mag = np.sqrt(re * re + im * im)                                          # [T, 513]
    mel = (mag @ fb).T
    energy = np.log1p(np.sqrt((mag * mag).sum(1)))
    fl = 2 * TAU_MAX
    yp = xp if len(xp) >= fl else np.pad(xp, (0, fl - len(xp)))
    P = (len(yp) - fl) // 256 + 1
    fr = yp[np.arange(P)[:, None] * 256 + np.arange(fl)[None, :]]
    sq = np.concatenate([np.zeros((P, 1)), np.cumsum(fr * fr, 1)], 1)
    r = np.stack([(fr[:, :fl - t] * fr[:, t:]).sum(1) for t in range(TAU_MAX)], 1)
    diff = sq[:, -1:] + (sq[:, ::-1][:, :TAU_MAX] - sq[:, :TAU_MAX]) - 2 * r
    d1 = diff[:, 1:]
    cmdf = d1 * np.arange(1, TAU_MAX) / np.maximum(np.cumsum(d1, 1), 1e-5)
    return mel, energy, cmdf[:, TAU_MIN:], T, P


def search64(c: np.ndarray):
    """torch-yin's decision on one float64 cmdf slice and whether it is fragile."""
    below = c < THR
    first = int(np.argmax(below)) if below.any() else 0
    dc = np.diff(c)
    upto = first if below.any() else len(c) - 1
    fragile = bool((np.abs(c[:upto + 1] - THR) < 1e-4).any())
    if first == 0:
        return 0, fragile
    slope = np.append(dc >= 0, True)
    tau = first + int(np.argmax(slope[first:]))
    fragile |= bool((np.abs(dc[first:min(tau + 1, len(dc))]) < 1e-6).any())
    return tau, fragile


def pitch_value(tau: int) -> np.float32:
    f = np.float32
    hz = (f(1) / f(tau + TAU_MIN + 1)) * f(SR) if tau > 0 else f(0)
    return (f(hz) - f(MEAN)) / f(STD)


def tau_of(value: np.float32) -> int:
    """The lag whose normalised pitch is `value` (bit for bit), -1 for none."""
    for t in range(0, TAU_MAX - 1 - TAU_MIN):
        if pitch_value(t).tobytes() == np.float32(value).tobytes():
            return t
    return -1


def check(out, waves, fb, expect=None, what=""):
    """Every bound of the module docstring for a batch; `expect` (the fixture's collated reference outputs) replaces the
    float64 values for mel / energy / pitch where given.  Returns the counts of fragile frames."""
    mel, mel_len = out["mel"].cpu().numpy(), out["mel_len"].cpu().numpy()
    pitch, energy = out["pitch"].cpu().numpy(), out["energy"].cpu().numpy()
    M = mel.shape[2]
    nfrag = ncheck = 0
    for b, w in enumerate(waves):
        w = w.numpy()
        S = len(w)
        if S < 256:
            assert mel_len[b] == 0 and not mel[b].any() and not pitch[b].any() and not energy[b].any(), what
            continue
        lin64, en64, cm, T, P = reference64(w, fb)
        assert mel_len[b] == T, f"{what}[{b}]: mel_len {mel_len[b]} != {T}"
        assert P == pitch_frames(S, TAU_MAX) and P <= T
        assert not mel[b, :, T:].any() and not pitch[b, T:].any() and not energy[b, T:].any(), f"{what}[{b}]: padding"
        lin = np.exp(mel[b, :, :T].astype(np.float64))
        fmax = np.maximum(lin64.max(0), 1e-30)
        big = lin64 >= 1e-2 * fmax
        ref_log = np.log(np.maximum(lin64, 1e-5)) if expect is None else expect["mel"][b, :, :T].astype(np.float64)
        err = np.abs(mel[b, :, :T] - ref_log)
        assert (err[big] <= 1e-4).all(), f"{what}[{b}]: log-mel error {err[big].max():.2e}"
        ref_lin = np.maximum(lin64, 1e-5) if expect is None else np.exp(ref_log)
        small = np.abs(np.maximum(lin, 1e-5) - ref_lin)
        assert (small[~big] <= 2e-6 * np.broadcast_to(fmax, lin.shape)[~big] + 1e-9).all(), f"{what}[{b}]: small mel"
        ref_en = en64 if expect is None else expect["energy"][b, :T].astype(np.float64)
        assert np.allclose(energy[b, :T], ref_en, rtol=1e-5, atol=1e-7), \
            f"{what}[{b}]: energy error {np.abs(energy[b, :T] - ref_en).max():.2e}"
        for t in range(P):
            tau64, fragile = search64(cm[t])
            ncheck += 1
            if fragile:
                nfrag += 1
                continue
            want = pitch_value(tau64) if expect is None else np.float32(expect["pitch"][b, t])
            assert np.float32(pitch[b, t]).tobytes() == want.tobytes(), \
                f"{what}[{b}] frame {t}: lag {tau_of(pitch[b, t])} != {tau64} (pitch {pitch[b, t]!r} vs {want!r})"
        assert not pitch[b, P:M].any()
    assert nfrag <= max(1, 0.02 * ncheck), f"{what}: {nfrag} of {ncheck} frames are fragile"
    return nfrag, ncheck


def run(feats, waves, nan_pad=True, strided=False):
    audio, lens = collate_audio(waves)
    if nan_pad:
        for i, w in enumerate(waves):
            audio[i, w.shape[0]:] = float("nan")
    if strided:                       # a row stride of S + 3: no float4 path
        wide = torch.full((audio.shape[0], audio.shape[1] + 3), float("nan"))
        wide[:, :audio.shape[1]] = audio
        a = wide.to(DEV)[:, :audio.shape[1]]
    else:
        a = audio.to(DEV)
    out = feats(a, lens.to(DEV))
    torch.cuda.synchronize()
    return out


# B, lengths (cycled kinds / amplitudes)
_EDGE = [256, 257, 281, 282, 283] + [k * 256 + o for k in (3, 17) for o in (0, 25, 26, 27)]
MATRIX = {
    "b1_one_frame": [256],
    "b1_long": [441088],
    "b3_pad_edge": [281, 282, 283],
    "b3_quirk": [40 * 256, 40 * 256 + 25, 40 * 256 + 26],
    "b3_long_mixed": [441088, 100000 + 27, 3000],
    "b14_edges": _EDGE,
    "b64_ragged": [int(v) for v in np.random.default_rng(5).integers(256, 24000, 64)],
}
_KINDS = [(k, a) for a in (0.9, 0.05, 1e-4) for k in synth.CLIP_KINDS]


def _waves(case):
    return [synth.make_clip(*_KINDS[(i * 7 + len(case)) % len(_KINDS)][:1], n, _KINDS[(i * 7 + len(case)) % len(_KINDS)][1])
            for i, n in enumerate(MATRIX[case])]


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("case", list(MATRIX))
def test_features_match_float64(case, strided):
    feats = extractor()
    waves = _waves(case)
    out = run(feats, waves, nan_pad=True, strided=strided)
    assert out["mel"].shape == (len(waves), 80, max(w.shape[0] for w in waves) // 256)
    check(out, waves, feats.fb.double().numpy(), what=case)


@pytest.mark.parametrize("case", list(synth.FEATURE_CASES))
def test_features_match_reference_fixture(case):
    import zlib
    g = np.load(os.path.join(ROOT, "tests", "golden", "features.npz"))
    waves = synth.make_feature_case(case)
    assert [zlib.crc32(w.numpy().tobytes()) for w in waves] == g[f"{case}_crc"].tolist(), "synth clips changed"
    feats = AcousticFeatures.from_config(config.ACOUSTIC_DATASET)
    out = run(feats, waves)
    assert out["mel"].shape == g[f"{case}_mel"].shape
    assert (out["mel_len"].cpu().numpy() == g[f"{case}_mel_len"]).all()
    expect = {k: g[f"{case}_{k}"] for k in ("mel", "pitch", "energy")}
    check(out, waves, feats.fb.double().numpy(), expect=expect, what=case)




def test_repeat_and_graph_replay_are_bit_identical():
    feats = extractor()
    waves = _waves("b64_ragged")
    audio, lens = collate_audio(waves)
    a, ln = audio.to(DEV), lens.to(DEV)
    o1 = {k: v.clone() for k, v in feats(a, ln).items()}
    o2 = feats(a, ln)
    out = feats.empty_outputs(*a.shape, DEV)
    feats(a, ln, out=out)                                  # (tables on the device, LDS reserved before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        feats(a, ln, out=out)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
        assert torch.equal(o1[k], out[k]), k


def test_extractor_issues_no_aten_compute_ops():
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

    feats = extractor()
    audio, lens = collate_audio(synth.make_feature_case("voices"))
    a, ln = audio.to(DEV), lens.to(DEV)
    feats(a, ln)                              # (the first call puts the tables on the device)
    torch.cuda.synchronize()
    with Spy():
        out = feats(a, ln)
    torch.cuda.synchronize()
    assert seen == [], f"PyTorch kernels inside the extractor: {sorted(set(seen))}"
    assert torch.isfinite(out["mel"]).all()


def test_out_of_range_lengths_give_empty_rows():
    """Below 256 samples (torch.stft raises there) or above S: mel_len 0 and all-zero rows; the other rows unaffected."""
    feats = extractor()
    w = synth.make_clip("harmonic", 3000, 0.5)
    audio = torch.stack([w, w, w, w]).to(DEV)
    lens = torch.tensor([3000, 255, 3001, -5], dtype=torch.int64, device=DEV)
    out = feats(audio, lens)
    torch.cuda.synchronize()
    assert out["mel_len"].tolist() == [11, 0, 0, 0]
    for k in ("mel", "pitch", "energy"):
        assert not out[k][1:].any()
    check({k: v[:1] for k, v in out.items()}, [w], feats.fb.double().numpy(), what="lens")


def test_disabled_outputs_are_not_written():
    feats = AcousticFeatures(sample_rate=SR, pitch=False, energy=False)
    audio, lens = collate_audio(synth.make_feature_case("edges"))
    out = feats(audio.to(DEV), lens.to(DEV))
    assert out["pitch"] is None and out["energy"] is None
    ref = extractor()(audio.to(DEV), lens.to(DEV))
    assert torch.equal(out["mel"], ref["mel"]) and torch.equal(out["mel_len"], ref["mel_len"])


# ------------------------------------------------------------------------------------------------------- training from audio
def _batch_from_audio(seed=9):
    """Three utterances of 160, 118 and 98 frames (the longest sets M = 160) with a synthetic text batch."""
    waves = [synth.make_clip(k, n, 0.5, seed) for k, n in (("harmonic", 160 * 256 + 100), ("chirp", 118 * 256), ("noise", 98 * 256 + 30))]
    audio, lens = collate_audio(waves)
    inp = synth.make_inputs(3, 52, 160, variable=True, seed=seed)
    return {"text": inp["text"].to(DEV), "text_len": inp["text_len"].to(DEV), "audio": audio.to(DEV),
            "audio_len": lens.to(DEV), "flow_x0": inp["flow_x0"].to(DEV), "flow_t": inp["flow_t"].to(DEV)}


@pytest.fixture(scope="module")
def state_dict():
    return synth.make_state_dict()


def _model(sd, train_mode=False):
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    m = AcousticModel.init(AcousticDims().model_config())
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    return m.train() if train_mode else m.eval()


def test_graphed_step_from_audio_matches_the_step_from_features(state_dict):
    """GraphedTrainStep(features=) on audio: after each of two replays step.features equals the eager extractor bit for bit,
    and total, losses and norm equal those of a step built without it on the extracted features."""
    from isp_tts_amd import train
    d = _batch_from_audio()
    feats = extractor()
    f = {k: v.clone() for k, v in feats(d["audio"], d["audio_len"]).items()}
    assert f["mel"].shape == (3, 80, 160) and f["mel_len"].tolist() == [160, 118, 98]

    def run(use_audio):
        torch.manual_seed(21)
        m = _model(state_dict)
        o = train.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, grad_clip=1.0)
        common = {k: d[k] for k in ("text", "text_len", "flow_x0", "flow_t")}
        if use_audio:
            batch = dict(common, audio=d["audio"], audio_len=d["audio_len"])
            step = train.GraphedTrainStep(m, o, batch, amp=True, features=feats)
        else:
            batch = dict(common, **f)
            step = train.GraphedTrainStep(m, o, batch, amp=True)
        res = []
        for _ in range(2):
            total, losses, norm = step()
            torch.cuda.synchronize()
            res.append([total.clone(), {k: v.clone() for k, v in losses.items()}, norm.clone()])
            if use_audio:
                for k in ("mel", "mel_len", "pitch", "energy"):
                    assert torch.equal(step.features[k], f[k]), k
        step.close()
        return res

    a, b = run(True), run(False)
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2])
        assert all(torch.equal(x[1][k], y[1][k]) for k in y[1])
        assert torch.isfinite(x[0])


def test_reference_loop_body_on_extracted_features(state_dict):
    """experiments/trainer.py:543-549 (model(**inputs), then the criterion) on the collated dict the extractor completes,
    against train.acoustic_train_forward on the same features: bit for bit."""
    from isp_tts_amd import train
    d = _batch_from_audio()
    f = extractor()(d["audio"], d["audio_len"])
    batch = {"text_vector": d["text"], "text_vector_len": d["text_len"], "speaker": None, **f}
    model, twin = _model(state_dict, True), _model(state_dict, True)
    criterion = train.AcousticModelLoss()
    torch.manual_seed(1234)
    inputs = model.prepare_inputs(batch)
    outputs = model(**inputs)
    loss, losses = criterion(inputs=inputs, outputs=outputs, step=0)
    torch.manual_seed(1234)
    _, total, terms = train.acoustic_train_forward(twin, d["text"], d["text_len"], f["mel"], f["mel_len"], f["pitch"], f["energy"])
    assert torch.isfinite(loss)
    assert torch.equal(loss.detach(), total.detach())
    assert all(torch.equal(losses[k].detach(), terms[k].detach()) for k in terms)
