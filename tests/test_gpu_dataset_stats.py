"""GPU: data.DatasetStats (ispk_feature_stats_f64) against the float64 restatement of tests/frontend_reference.py and the
reference's own results (tests/golden/dataset_stats.npz, tools/make_dataset_stats_golden.py).

Per utterance: kept count, min and max exactly; mean and M2 within 1e-9 relative.  Pooled: mean and std within 1e-9 relative
of a float64 two-pass over the kept values.  1e-9 is derived: float64 accumulation over at most 2^20 values has
gamma_n = n 2^-53 ~ 1.2e-10, and Chan's M2 update has no cancellation.  The reference's fp32 StandardScaler agrees with
float64 to 1e-4 relative (tests/test_audio_frontend_host.py); the kernel must be at least as close to float64 as it is."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import frontend_reference as fr
from isp_tts_amd import synth
from isp_tts_amd.data import AcousticFeatures, DatasetStats, Resampler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-9
NAMES = ("pitch", "energy")


def close(a, b):
    return abs(a - b) <= RTOL * abs(b)


def on_device(d, nan_pad=True):
    p, e = d["pitch"].clone(), d["energy"].clone()
    if nan_pad:                               # nothing at or past mel_len is read
        for b, n in enumerate(d["mel_len"].tolist()):
            p[b, n:] = float("nan")
            e[b, n:] = float("nan")
    return p.to(DEV), e.to(DEV), d["mel_len"].to(DEV)


def check_partials(partials, d, what):
    part = partials.cpu().numpy()
    for b, n in enumerate(d["mel_len"].tolist()):
        for f, name in enumerate(NAMES):
            cnt, mean, m2, mn, mx = fr.partial64(d[name][b, :n].numpy(), name == "pitch")
            got = part[b, f]
            assert got[0] == cnt, f"{what}[{b}] {name}: kept {got[0]} != {cnt}"
            assert got[3] == mn and got[4] == mx, f"{what}[{b}] {name}: min / max {got[3]}, {got[4]} != {mn}, {mx}"
            assert close(got[1], mean), f"{what}[{b}] {name}: mean {got[1]!r} vs {mean!r}"
            assert close(got[2], m2), f"{what}[{b}] {name}: M2 {got[2]!r} vs {m2!r}"


def check_pooled(res, batches, what, golden=None):
    for name in NAMES:
        rows = [r for d in batches for r in d[name].numpy()]
        lens = [n for d in batches for n in d["mel_len"].tolist()]
        cnt, mn, mx, mean, std = fr.pooled64(rows, lens, name == "pitch")
        got = getattr(res, name)
        print(f"{what} {name}: count {got.count} mean {got.mean!r} ({abs(got.mean - mean) / abs(mean):.1e}) "
              f"std {got.std!r} ({abs(got.std - std) / std:.1e})")
        assert got.count == cnt and got.min == mn and got.max == mx, f"{what} {name}"
        assert close(got.mean, mean) and close(got.std, std), f"{what} {name}: {got} vs mean {mean!r} std {std!r}"
        if golden is not None:
            ref = golden[name]
            assert ref[0] == got.min and ref[1] == got.max
            assert abs(got.mean - ref[2]) <= 1e-4 * abs(ref[2]) and abs(got.std - ref[3]) <= 1e-4 * ref[3]
            assert abs(got.mean - mean) <= abs(ref[2] - mean) + RTOL * abs(mean), f"{what} {name}: farther from float64 than the reference"
            assert abs(got.std - std) <= abs(ref[3] - std) + RTOL * std, f"{what} {name}: farther from float64 than the reference"


@pytest.mark.parametrize("case", synth.STATS_CASES)
def test_cases_match_float64_and_the_reference(case):
    g = np.load(os.path.join(ROOT, "tests", "golden", "dataset_stats.npz"))
    d = synth.make_stats_case(case)
    stats = DatasetStats(DEV)
    stats.update(*on_device(d))
    torch.cuda.synchronize()
    assert stats.partials.shape == (d["mel_len"].shape[0], 2, 5)
    assert (stats.partials[:, :, 0].cpu().numpy() == g[f"{case}_kept"]).all(), "kept counts differ from the reference's"
    check_partials(stats.partials, d, case)
    res = stats.result()
    check_pooled(res, [d], case, golden={n: g[f"{case}_{n}"] for n in NAMES})
    assert set(res.to_dict()) == {"pitch", "energy"} and res.to_dict()["pitch"]["mean"] == res.pitch.mean
    assert res.counts == {"pitch": int(g[f"{case}_kept"][:, 0].sum()), "energy": int(g[f"{case}_kept"][:, 1].sum())}


def test_quirks():
    """75 % or more unvoiced: no pitch; a constant feature, a single frame, a NaN, mel_len 0: nothing.  (0, 0, 0, +inf, -inf)."""
    empty = [0.0, 0.0, 0.0, float("inf"), float("-inf")]
    for case, rows in (("mostly_unvoiced", [(0, 0), (1, 0), (2, 0), (3, 0)]), ("constant", [(0, 1), (1, 0), (2, 0), (2, 1)]),
                       ("single_frame", [(0, 0), (0, 1), (1, 0), (1, 1)]), ("nan", [(0, 0), (1, 1)]),
                       ("empty_len", [(0, 0), (0, 1), (2, 0), (2, 1)])):
        d = synth.make_stats_case(case)
        stats = DatasetStats(DEV)
        stats.update(*on_device(d))
        part = stats.partials.cpu()
        for b, f in rows:
            assert part[b, f].tolist() == empty, f"{case}[{b}] {NAMES[f]}: {part[b, f].tolist()}"
        others = [(b, f) for b in range(part.shape[0]) for f in (0, 1) if (b, f) not in rows]
        assert all(part[b, f, 0] > 0 for b, f in others), case


def test_nothing_kept_raises_and_lengths_out_of_range_count_as_empty():
    d = synth.make_stats_case("mostly_unvoiced")
    p, e, ln = on_device(d)
    stats = DatasetStats(DEV)
    with pytest.raises(ValueError, match="pitch"):
        stats.result()
    stats.update(p[:4], e[:4], ln[:4])
    with pytest.raises(ValueError, match="no pitch value"):
        stats.result()
    stats.reset()
    bad = ln.clone()
    bad[0], bad[1] = p.shape[1] + 1, -3
    stats.update(p, e, bad)
    assert not stats.partials[:2, :, 0].any()
    assert stats.result().pitch.count == int(stats.partials[4, 0, 0])


def test_two_batches_equal_one_and_reset_works():
    d = synth.make_stats_case("voices")
    p, e, ln = on_device(d)
    one = DatasetStats(DEV)
    one.update(p, e, ln)
    want = one.result()
    two = DatasetStats(DEV)
    two.update(p[:23], e[:23], ln[:23])
    two.update(p[23:], e[23:], ln[23:])
    got = two.result()
    for name in NAMES:
        a, b = getattr(got, name), getattr(want, name)
        assert (a.count, a.min, a.max) == (b.count, b.min, b.max)
        assert close(a.mean, b.mean) and close(a.std, b.std)
    check_pooled(got, [d], "two batches")
    s0 = one.state.clone()
    small = synth.make_stats_case("empty_len")
    one.update(*on_device(small))
    merged = one.result()
    check_pooled(merged, [d, small], "voices + empty_len")
    one.reset()
    with pytest.raises(ValueError):
        one.result()
    one.update(p, e, ln)
    assert torch.equal(one.state, s0), "reset() then the same batch does not reproduce the state"


def test_repeats_and_graph_replay_are_bit_identical():
    d = synth.make_stats_case("voices")
    p, e, ln = on_device(d)
    a, b = DatasetStats(DEV), DatasetStats(DEV)
    a.update(p, e, ln)
    b.update(p, e, ln)
    assert torch.equal(a.state, b.state) and torch.equal(a.partials, b.partials)
    c = DatasetStats(DEV)
    c.update(p, e, ln)                                  # (allocates the partials before the capture)
    c.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.update(p, e, ln)
    c.reset()
    c.partials.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a.state, c.state) and torch.equal(a.partials, c.partials)
    g.replay()
    a.update(p, e, ln)
    torch.cuda.synchronize()
    assert torch.equal(a.state, c.state)


def test_row_strided_inputs():
    d = synth.make_stats_case("nan")
    p, e, ln = on_device(d)
    wide_p = torch.full((p.shape[0], p.shape[1] + 5), float("nan"), device=DEV)
    wide_e = wide_p.clone()
    wide_p[:, :p.shape[1]], wide_e[:, :p.shape[1]] = p, e
    a, b = DatasetStats(DEV), DatasetStats(DEV)
    a.update(p, e, ln)
    b.update(wide_p[:, :p.shape[1]], wide_e[:, :p.shape[1]], ln)
    assert torch.equal(a.state, b.state) and torch.equal(a.partials, b.partials)


def test_update_issues_no_aten_compute_ops():
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

    p, e, ln = on_device(synth.make_stats_case("voices"))
    with Spy():
        stats = DatasetStats(DEV)
        stats.update(p, e, ln)
        stats.reset()
        stats.update(p, e, ln)
    torch.cuda.synchronize()
    assert seen == [], f"PyTorch kernels inside DatasetStats: {sorted(set(seen))}"
    assert stats.result().pitch.count > 0


def test_from_48k_audio_to_statistics():
    """make_feature_case("voices") clips made at 48 kHz -> Resampler -> AcousticFeatures(mean 0, std 1) -> DatasetStats equals
    DatasetStats fed the extractor's own arrays, bit for bit, and the float64 restatement on those arrays; the result then
    normalises the pitch through set_pitch_stats."""
    rs = Resampler(48000, 22050)
    feats = AcousticFeatures(sample_rate=22050, pitch_mean=0.0, pitch_std=1.0)
    waves = [synth.make_clip(k, (n * 320) // 147, amp, sample_rate=48000) for k, n, amp in synth.FEATURE_CASES["voices"]]
    S = max(w.shape[0] for w in waves)
    audio = torch.zeros(len(waves), S)
    for i, w in enumerate(waves):
        audio[i, :w.shape[0]] = w
    lens = torch.tensor([w.shape[0] for w in waves], dtype=torch.int64, device=DEV)
    chain = DatasetStats(DEV)
    out = feats(*rs(audio.to(DEV), lens))
    chain.update(out["pitch"], out["energy"], out["mel_len"])
    arrays = {k: out[k].cpu() for k in ("pitch", "energy", "mel_len")}
    direct = DatasetStats(DEV)
    direct.update(arrays["pitch"].to(DEV), arrays["energy"].to(DEV), arrays["mel_len"].to(DEV))
    assert torch.equal(chain.state, direct.state) and torch.equal(chain.partials, direct.partials)
    res = chain.result()
    check_pooled(res, [arrays], "48k chain")
    assert 60.0 < res.pitch.mean < 500.0 and res.pitch.std > 0
    feats.set_pitch_stats(res.pitch.mean, res.pitch.std)
    norm = feats(*rs(audio.to(DEV), lens))["pitch"]
    b, t = 0, 5
    want = (np.float32(arrays["pitch"][b, t]) - np.float32(res.pitch.mean)) / np.float32(res.pitch.std)
    assert abs(float(norm[b, t]) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
