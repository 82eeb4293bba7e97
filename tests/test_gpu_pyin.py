"""GPU: the pitch tracker (data.PitchTracker: csrc/pyin.hip, ispk_pyin_observe_f32 / ispk_pyin_decode_f64) against the float64
restatement of tests/pyin_reference.py.

Decode, exact.  Log-observations and transition tables that are multiples of 2^-8 in a small range: every sum of the recursion is
exact in float64, so states, voiced flags and log_prob must EQUAL the reference's, ties (planted: few distinct values, a flat top of
the window) included.

Observe.  A row depends on the samples only through comparisons and one rounding, so a frame is *fragile* when, in float64, one of
them lies within a stated delta of its decision point; every other frame matches within 1e-6 absolute (a few fp32 roundings of sums
of at most 100 prior terms, each below 0.072).  The deltas.  The device's cmnd differs from float64 by the error of its fp32
cross-correlation: three 1,024-point transforms of five radix-4 passes and two splits, about 8 eps32 of the window's energy E0 in
c(tau); cmnd = d / mean(d) with mean(d) about 2 E0, and d = .. - 2 c, so |delta cmnd| <= 8 eps32 = 9.5e-7.
  DELTA_H = 2e-6   a trough height against a threshold (that bound, doubled for the running mean's share)
  2 DELTA_H        the neighbour comparison that defines a trough (two such values)
  bin              the pre-rounding value 12 bps log2(sr / (lag + shift) / f_min) moves by 12 bps / ln 2 * |d shift| / lag with
                   |d shift| <= 4 DELTA_H / |a| (shift = -b / a, |shift| <= 1 / 2, a and b sums of such values); fragile when it lies
                   closer than that (+ 1e-9) to a half-integer.
At most 5 % of the frames may be excluded this way (tests/test_pyin_host.py: the restatement with an fp32 difference function gives
the float64 rows on all 78 frames of the clip).

End to end on the same clip: the device's own rows go to the reference decoder; the device's path, re-scored in float64, is within
1e-9 |optimum| of the optimum (insensitive to ties among the equal unvoiced states); voiced flags and, where both are voiced, bins
agree on all but 2 % of the frames.  A ragged batch gives each item the bits it gets alone; a second call and a graph replay repeat
the bits; AcousticFeatures(pitch_method="pyin") holds the normalised tracker's bits; the default method is bit-identical to the
extractor's own launch."""
import math

import numpy as np
import pytest
import torch

import pyin_reference as R
from isp_tts_amd import config, runtime, synth
from isp_tts_amd.data import AcousticFeatures, PitchTracker, collate_audio
from isp_tts_amd.data.pitch import transition_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
SR = 22050
F_MIN, F_MAX, BPS = 55.0, 880.0, 10
NB, WIDTH = 481, 51
DELTA_H = 2e-6
S = 20000
LENS = (S, 13131, 200)        # whole; not a multiple of 256 (51 frames); below 256 samples (no frames)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


@pytest.fixture(scope="module")
def clip():
    """(audio fp32 [3, S] on the host, lengths, the float64 rows and margins of items 0 and 1) - computed once, left unchanged."""
    x = R.clip(SR, S)
    audio = np.zeros((3, S), np.float32)
    for b, n in enumerate(LENS):
        audio[b, :n] = x[:n]
    audio[2, LENS[2]:] = 7.0             # (nothing at or past a length is read)
    audio[1, LENS[1]:] = -3.0
    ref = [R.observe_item(audio[b, :LENS[b]], SR, F_MIN, F_MAX, BPS) for b in range(2)]
    return torch.from_numpy(audio), torch.tensor(LENS, dtype=torch.int64), ref


@pytest.fixture(scope="module")
def tracked(clip):
    """The device's results on the clip batch, once: (tracker, its `out` dict with every tensor, the returned dict)."""
    audio, lens, _ = clip
    t = PitchTracker(SR, F_MIN, F_MAX, BPS)
    assert (t.n_bins, t.width, t.min_period, t.max_period) == (NB, WIDTH, 25, 401)
    out = t.empty_outputs(3, S, DEV)
    for v in out.values():
        v.view(torch.uint8).fill_(0x5b)     # (every element is written)
    r = t(audio.to(DEV), lens.to(DEV), out=out)
    torch.cuda.synchronize()
    return t, out, r


# ------------------------------------------------------------------------------------------------------------------ decode
def _dyadic_case(nb, width, m, seed):
    g = np.random.default_rng(seed)
    h = (width - 1) // 2
    q = 1.0 / 256.0
    lens = [m, 0, (m + 1) // 2]
    # few distinct values (ties between states), some frames entirely flat (ties between whole paths)
    logobs = g.integers(-12, 1, size=(3, m, 2 * nb)).astype(np.float64) * 0.5 + g.integers(-3, 1, size=(3, m, 1)) * q
    logobs[0, m // 2] = -1.0
    logobs[:, :, nb:] = np.minimum(logobs[:, :, nb:], -2.0) + g.integers(0, 2, size=(3, m, 1)) * 1.5
    logtri = -np.maximum(np.abs(np.arange(width) - h) - 1, 0) * 0.25            # a flat top of three: neighbours tie
    lognorm = g.integers(0, 64, size=nb) * q
    tables = (logtri, lognorm, -3 * q, -4.5, -7.0)
    trans = np.concatenate([logtri, lognorm, [tables[2], tables[3], tables[4]]])
    return lens, logobs, tables, trans


@pytest.mark.parametrize("m", [1, 2, 40])
@pytest.mark.parametrize("nb, width", [(33, 7), (130, 21), (33, 127)])
def test_decode_is_exact_on_dyadic_scores(nb, width, m):
    lens, logobs, tables, trans = _dyadic_case(nb, width, m, seed=1000 * nb + 10 * width + m)
    obs = torch.from_numpy(logobs).to(DEV)
    r = runtime.pyin_decode(obs, torch.tensor(lens, dtype=torch.int64, device=DEV), torch.from_numpy(trans).to(DEV), width,
                            F_MIN, BPS)
    torch.cuda.synchronize()
    assert r["frames"].tolist() == lens
    for b, n in enumerate(lens):
        states, logp = R.viterbi(logobs[b, :n], tables, width)
        got = r["state"][b].cpu().numpy()
        assert np.array_equal(got[:n], states), (b, np.nonzero(got[:n] != states)[0][:5])
        assert (got[n:] == -1).all()
        assert r["log_prob"][b].item() == logp
        voiced = r["voiced"][b].cpu().numpy()
        assert np.array_equal(voiced[:n], (states < nb).astype(np.int32)) and not voiced[n:].any()
        f0 = r["f0"][b].cpu().numpy()
        want = R.f0_of(states, F_MIN, nb, BPS).astype(np.float32)
        assert np.abs(f0[:n] - want).max(initial=0.0) <= np.spacing(np.float32(F_MIN * 2 ** (nb / 120.0))) and not f0[n:].any()
        assert ((f0[:n] == 0) == (states >= nb)).all()
        assert not r["voiced_prob"][b].any()
        # the path is a path of the model: re-scored, it has the decoder's own log-probability
        assert n == 0 or R.path_log_prob(states, logobs[b, :n], tables, width) == logp


def test_decode_without_lengths_takes_every_frame():
    lens, logobs, tables, trans = _dyadic_case(33, 7, 5, seed=4)
    r = runtime.pyin_decode(torch.from_numpy(logobs).to(DEV), None, torch.from_numpy(trans).to(DEV), 7, F_MIN, BPS)
    torch.cuda.synchronize()
    assert r["frames"].tolist() == [5, 5, 5]
    for b in range(3):
        states, logp = R.viterbi(logobs[b], tables, 7)
        assert np.array_equal(r["state"][b].cpu().numpy(), states) and r["log_prob"][b].item() == logp


# ----------------------------------------------------------------------------------------------------------------- observe
def _fragile(m):
    if m["threshold"] < DELTA_H or m["neighbour"] < 2 * DELTA_H:
        return True
    return any(dist < 12 * BPS / math.log(2.0) * (4 * DELTA_H / abs(a)) / lag + 1e-9 for dist, a, lag in m["bin"])


def test_observation_rows_match_float64(clip, tracked):
    _, _, ref = clip
    _, out, r = tracked
    assert runtime.lib().ispk_pyin_frames_per_block() == 8            # 78 and 51 frames end inside a workgroup's eight
    assert r["frames"].tolist() == [78, 51, 0] == [R.frames_of(n) for n in LENS]
    obs = out["obs"].cpu().numpy().astype(np.float64)
    assert obs.shape == (3, 78, NB)
    assert not obs[2].any() and not obs[1, 51:].any()
    total = excluded = 0
    for b, (rows, margins) in enumerate(ref):
        n = len(rows)
        frag = np.array([_fragile(m) for m in margins])
        err = np.abs(obs[b, :n] - rows).max(axis=1)
        total, excluded = total + n, excluded + int(frag.sum())
        print(f"item {b}: {n} frames, {int(frag.sum())} fragile, worst error on the others {err[~frag].max():.3e}, "
              f"on the fragile ones {err[frag].max(initial=0.0):.3e}; voiced rows {(rows.sum(axis=1) > 0.5).sum()}")
        assert frag.sum() <= 0.05 * n, f"item {b}: {int(frag.sum())} of {n} frames are fragile"
        bad = np.nonzero(~frag & (err > 1e-6))[0]
        assert len(bad) == 0, (b, bad[:8], err[bad[:8]])
    assert excluded <= 0.05 * total


# -------------------------------------------------------------------------------------------------------------- end to end
def test_path_is_optimal_for_the_device_rows(clip, tracked):
    _, out, r = tracked
    tables = R.transition_tables(NB, WIDTH)
    assert np.array_equal(transition_table(NB, WIDTH).numpy()[:WIDTH], tables[0])
    obs = out["obs"].cpu().numpy()
    for b, n in enumerate((78, 51)):
        logobs, vp = R.log_observations(obs[b, :n])
        states, opt = R.viterbi(logobs, tables, WIDTH)
        got = out["state"][b, :n].cpu().numpy()
        rescored = R.path_log_prob(got, logobs, tables, WIDTH)
        print(f"item {b}: optimum {opt:.12f}, the device's path re-scored {rescored:.12f}, its own {r['log_prob'][b].item():.12f}")
        assert abs(rescored - opt) <= 1e-9 * abs(opt)
        assert abs(r["log_prob"][b].item() - opt) <= 1e-9 * abs(opt)
        dv, rv = got < NB, states < NB
        assert (dv != rv).sum() <= 0.02 * n
        both = dv & rv
        assert both.sum() >= 20 and (got[both] != states[both]).sum() <= 0.02 * both.sum()      # (42 and 23 frames lie inside the tone)
        assert np.array_equal(r["voiced"][b, :n].cpu().numpy().astype(bool), dv) and not r["voiced"][b, n:].any()
        assert np.abs(r["voiced_prob"][b, :n].cpu().numpy() - vp).max() <= 1e-6 and not r["voiced_prob"][b, n:].any()
        f0 = r["f0"][b].cpu().numpy()
        want = R.f0_of(got, F_MIN, NB, BPS)
        assert np.abs(f0[:n] - want).max() <= np.spacing(np.float32(F_MAX)) and not f0[n:].any()
        # the glide stays inside 140 Hz * 2^+-0.31 on the frames that lie inside the tone
        inside = [t for t in range(n) if 2048 <= 256 * t - 384 and 256 * t + 1664 <= min(LENS[b], S - 2048)
                  and not (256 * t - 384 < 10500 and 256 * t + 1664 > 9500)]
        inside = np.array(inside)
        sung = inside[dv[inside]]
        assert len(inside) >= 20 and len(sung) >= len(inside) - math.ceil(0.02 * n)
        assert (f0[sung] > 140 * 2 ** -0.32).all() and (f0[sung] < 140 * 2 ** 0.32).all()
    assert r["frames"].tolist() == [78, 51, 0] and r["log_prob"][2].item() == 0.0 and (out["state"][2] == -1).all()


def test_tracker_follows_the_reference_track(clip, tracked):
    """The whole float64 reference (its own rows, its own decode) against the device: flags and bins agree on all but 2 %."""
    audio, _, _ = clip
    _, out, _ = tracked
    _, _, states, _, _ = R.track(audio[0].numpy(), SR, F_MIN, F_MAX, BPS)
    got = out["state"][0].cpu().numpy()
    dv, rv = got < NB, states < NB
    assert (dv != rv).sum() <= 0.02 * 78
    both = dv & rv
    assert (got[both] != states[both]).sum() <= 0.02 * both.sum()


def test_ragged_batch_gives_each_item_its_own_bits(clip, tracked):
    audio, lens, _ = clip
    t, out, r = tracked
    for b in (0, 1, 2):
        n = LENS[b]
        alone = t.empty_outputs(1, max(n, 256), DEV)
        a = torch.zeros(1, max(n, 256))
        a[0, :n] = audio[b, :n]
        ra = t(a.to(DEV), torch.tensor([n], dtype=torch.int64, device=DEV), out=alone)
        torch.cuda.synchronize()
        m = R.frames_of(n)
        assert ra["frames"].tolist() == [m]
        assert bits(alone["obs"][0, :m]) == bits(out["obs"][b, :m])
        for k in ("f0", "voiced", "voiced_prob"):
            assert bits(ra[k][0, :m]) == bits(r[k][b, :m]), (b, k)
        assert bits(alone["state"][0, :m]) == bits(out["state"][b, :m]) and bits(ra["log_prob"]) == bits(r["log_prob"][b:b + 1])


def test_second_call_and_graph_replay_repeat_the_bits(clip, tracked):
    audio, lens, _ = clip
    t, out, r = tracked
    t = t.normalised(166.6177, 62.5423)
    a, ln = audio.to(DEV), lens.to(DEV)
    o2 = t.empty_outputs(3, S, DEV)
    r2 = t(a, ln, out=o2)
    torch.cuda.synchronize()
    keys = ("obs", "state", "f0", "voiced", "voiced_prob", "frames", "log_prob")
    for k in keys:
        assert bits(o2[k]) == bits(out[k]), k
    first = {k: v.clone() for k, v in o2.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t(a, ln, out=o2)
    for k in keys + ("pitch",):
        o2[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in keys + ("pitch",):
        assert bits(o2[k]) == bits(first[k]), k
    # the normalised contour: (f0 - mean) / std in fp32, unvoiced frames at -mean / std, zeros past the frames
    f0 = r["f0"].cpu()
    want = (f0 - torch.tensor(166.6177)) / torch.tensor(62.5423)
    for b, n in enumerate((78, 51, 0)):
        want[b, n:] = 0.0
    assert bits(r2["pitch"]) == bits(want)


# ----------------------------------------------------------------------------------------------------------- the extractor
def _dataset(method):
    import copy
    d = copy.deepcopy(config.ACOUSTIC_DATASET)
    d["pitch"]["method"] = method
    return d


def test_extractor_with_pyin_holds_the_normalised_tracker(clip):
    audio, lens, _ = clip
    a, ln = audio.to(DEV), lens.to(DEV)
    feats = AcousticFeatures.from_config(_dataset("pyin"))
    base = AcousticFeatures.from_config(_dataset("torch-yin"))
    out = feats(a, ln)
    ref = base(a, ln)
    torch.cuda.synchronize()
    t = PitchTracker(SR, f_min=40.0, f_max=800.0).normalised(feats.pitch_mean, feats.pitch_std)
    want = t(a, ln)
    torch.cuda.synchronize()
    assert out["pitch"].shape == (3, 78) and bits(out["pitch"]) == bits(want["pitch"])
    assert out["pyin"]["pitch"] is out["pitch"] and bits(out["pyin"]["f0"]) == bits(want["f0"])
    for k in ("mel", "mel_len", "energy"):
        assert bits(out[k]) == bits(ref[k]), k
    assert not torch.equal(out["pitch"], ref["pitch"])
    assert out["mel_len"].tolist() == want["frames"].tolist() == [78, 51, 0]
    # new statistics reach the next call
    feats.set_pitch_stats(100.0, 50.0)
    again = feats(a, ln)
    torch.cuda.synchronize()
    assert bits(again["pitch"]) == bits(PitchTracker(SR, f_min=40.0, f_max=800.0).normalised(100.0, 50.0)(a, ln)["pitch"])


def test_default_method_is_the_extractors_own_launch(clip):
    """pitch_method left alone: every output is what runtime.audio_features (the one launch the extractor made before) writes."""
    audio, lens, _ = clip
    a, ln = audio.to(DEV), lens.to(DEV)
    feats = AcousticFeatures.from_config(config.ACOUSTIC_DATASET)
    assert feats.pitch_method == "torch-yin" and feats.tracker is None
    out = feats(a, ln)
    assert set(out) == {"mel", "mel_len", "pitch", "energy"}
    direct = {"mel": torch.empty_like(out["mel"]), "mel_len": torch.empty_like(out["mel_len"]),
              "pitch": torch.empty_like(out["pitch"]), "energy": torch.empty_like(out["energy"])}
    tables, fb_index = feats.device_tables(DEV)
    runtime.audio_features(a, ln, tables, fb_index, direct["mel"], direct["mel_len"], direct["pitch"], direct["energy"],
                           feats.tau_min, feats.tau_max, float(feats.sample_rate), feats.threshold, feats.pitch_mean,
                           feats.pitch_std)
    torch.cuda.synchronize()
    for k in direct:
        assert bits(out[k]) == bits(direct[k]), k


def test_extractor_with_pyin_issues_no_aten_compute_ops(clip):
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

    audio, lens, _ = clip
    a, ln = audio.to(DEV), lens.to(DEV)
    feats = AcousticFeatures.from_config(_dataset("pyin"))
    out = feats.empty_outputs(3, S, DEV)
    feats(a, ln, out=out)
    torch.cuda.synchronize()
    with Spy():
        feats(a, ln, out=out)
    torch.cuda.synchronize()
    assert seen == [], f"PyTorch kernels inside the extractor: {sorted(set(seen))}"


def test_graphed_step_captures_the_pyin_extractor():
    """GraphedTrainStep(features=) with pitch_method="pyin": after each of two replays step.features holds the eager extractor's
    bits, the tracker's contour among them, and the step's loss is finite."""
    from isp_tts_amd import train
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    waves = [synth.make_clip(k, n, 0.5, 9) for k, n in (("harmonic", 160 * 256 + 100), ("chirp", 118 * 256), ("noise", 98 * 256 + 30))]
    audio, lens = collate_audio(waves)
    inp = synth.make_inputs(3, 52, 160, variable=True, seed=9)
    batch = {"text": inp["text"].to(DEV), "text_len": inp["text_len"].to(DEV), "audio": audio.to(DEV), "audio_len": lens.to(DEV),
             "flow_x0": inp["flow_x0"].to(DEV), "flow_t": inp["flow_t"].to(DEV)}
    feats = AcousticFeatures.from_config(_dataset("pyin"))
    f = feats(batch["audio"], batch["audio_len"])
    f = {k: f[k].clone() for k in ("mel", "mel_len", "pitch", "energy")}
    assert f["mel_len"].tolist() == [160, 118, 98]
    torch.manual_seed(21)
    m = AcousticModel.init(AcousticDims().model_config())
    m.load_state_dict(synth.make_state_dict(), strict=True)
    m = m.to(DEV).eval()
    o = train.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, grad_clip=1.0)
    step = train.GraphedTrainStep(m, o, batch, amp=True, features=feats)
    try:
        for _ in range(2):
            total, _, _ = step()
            torch.cuda.synchronize()
            assert torch.isfinite(total)
            for k in f:
                assert bits(step.features[k]) == bits(f[k]), k
    finally:
        step.close()
