"""CPU: the audio front end's host side - the resampler's tap table against its float64 definition, the output-length rule,
the definition's indexing against scipy's independent polyphase application, the statistics generators' safety margin, and
the argument checks of ispk_resample_f32 / ispk_feature_stats_f64, which run before any launch."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

import frontend_reference as fr
from isp_tts_amd import runtime, synth
from isp_tts_amd.data import AcousticFeatures, AudioFrontEnd, DatasetStats, Resampler, resampled_length

PAIRS = [(a, b) for a in fr.RATES for b in fr.RATES if a != b]


@pytest.mark.parametrize("orig,new", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_tap_table_is_the_float64_definition_rounded_once(orig, new):
    """Every stored tap within 2^-24 relative of the dense definition; every tap the compact table drops (or zero-fills) is
    below 1e-30; the runs stay inside the dense range."""
    rs = Resampler(orig, new)
    k, o, n, width = fr.dense_taps(orig, new)
    assert (rs.o, rs.n, rs.width) == (o, n, width)
    taps, first = rs.taps.double().numpy(), rs.first.numpy()
    T, J = taps.shape[1], k.shape[1]
    assert taps.shape == (n, T) and first.shape == (n,) and T == rs.T and taps.size <= 12288
    assert (first >= 0).all() and (first + T <= J).all()
    covered = np.zeros_like(k, dtype=bool)
    for p in range(n):
        want = k[p, first[p]:first[p] + T]
        stored = taps[p] != 0
        assert (np.abs(taps[p][stored] - want[stored]) <= 2.0 ** -24 * np.abs(want[stored])).all(), f"phase {p}"
        covered[p, first[p]:first[p] + T] = stored
    assert np.abs(k[~covered]).max(initial=0.0) < 1e-30
    assert T == fr.taps_per_phase(k, 6, o, n, width)


def test_every_supported_pair_fits_and_a_huge_table_is_refused():
    sizes = {(a, b): Resampler(a, b).taps.numel() for a, b in PAIRS}
    assert max(sizes.values()) <= 12288
    assert sizes[(32000, 22050)] == 7938
    with pytest.raises(NotImplementedError, match="floats|phases"):
        Resampler(44100, 44099)
    with pytest.raises(ValueError):
        Resampler(0, 22050)


@pytest.mark.parametrize("orig,new", [(48000, 22050), (22050, 24000), (44100, 8000), (8000, 44100)])
def test_out_len_is_ceil(orig, new):
    rs = Resampler(orig, new)
    o, n = rs.o, rs.n
    for base in (0, 1, 2, 7):
        for d in (-2, -1, 0, 1, 2):
            length = base * o + d
            if length < 0:
                continue
            want = math.ceil(n * length / o)
            assert resampled_length(length, o, n) == -((-n * length) // o) == want == fr.out_length(length, o, n)
            assert rs.out_samples(length) == want
            x = np.ones(length)
            assert len(fr.resample64(x, *fr.dense_taps(orig, new))[0]) == want


@pytest.mark.parametrize("orig,new", [(48000, 22050), (44100, 22050), (22050, 24000), (16000, 22050), (32000, 22050)])
def test_direct_sum_matches_scipy_upfirdn(orig, new):
    """The definition's indexing, phase order and pads against scipy.signal.upfirdn(h, x_pad, up=n, down=o), an independent
    polyphase application: y[m'] = sum_i x_pad[i] h[m' o - i n].  Output m = q n + p of the definition reads x_pad[q o + j]
    with k[p, j], i.e. h[m o - (q o + j) n] = h[p o - j n]; with the taps laid out as h[off + p o - j n] = k[p, j] (o and n
    are coprime, so no two taps share a slot; off a multiple of o) the definition's output m is upfirdn's m + off / o."""
    from scipy.signal import upfirdn
    k, o, n, width = fr.dense_taps(orig, new)
    J = k.shape[1]
    off = -(-(J - 1) * n // o) * o
    h = np.zeros(off + (n - 1) * o + 1)
    for p in range(n):
        h[off + p * o - np.arange(J) * n] = k[p]
    assert np.count_nonzero(h) == np.count_nonzero(k)
    rng = np.random.default_rng(orig + new)
    for length in (1, o - 1, o, o + 1, 3 * o + 1, 5 * o - 1, 1000):
        x = rng.standard_normal(length)
        y, _ = fr.resample64(x, k, o, n, width)
        xp = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
        full = upfirdn(h, xp, up=n, down=o)
        got = full[off // o:off // o + len(y)]
        peak = max(np.abs(full).max(), 1e-300)
        assert len(got) == len(y) and np.abs(got - y).max() <= 1e-12 * peak, \
            f"{orig}->{new} len {length}: {np.abs(got - y).max() / peak:.2e}"


def test_sine_comes_out_as_a_sine():
    """Sanity of the restatement's time scale: a unit 1 kHz sine, 48k -> 22.05k, away from the edges, stays within 1e-3 of the
    analytic sine at the new rate (the bar a different filter design, scipy's resample_poly, also meets; the windowed sinc's
    passband error at 1 kHz is about 1e-4)."""
    k, o, n, width = fr.dense_taps(48000, 22050)
    x = np.sin(2 * np.pi * 1000.0 * np.arange(9600) / 48000.0)
    y, _ = fr.resample64(x, k, o, n, width)
    m = np.arange(len(y))
    want = np.sin(2 * np.pi * 1000.0 * m / 22050.0)
    assert np.abs(y - want)[200:-200].max() < 1e-3


@pytest.mark.parametrize("case", synth.STATS_CASES)
def test_stats_cases_are_safe_by_construction(case):
    """No value within 2^-20 (|p25| + |p75|) of a fence unless IQR == 0: the count of such values is 0, so kept counts are
    comparable exactly.  The fixture's kept counts (the reference's fp32 decisions) equal the float64 ones."""
    d = synth.make_stats_case(case)
    g = np.load(os.path.join(ROOT, "tests", "golden", "dataset_stats.npz"))
    import zlib
    assert [zlib.crc32(np.ascontiguousarray(d[k].numpy()).tobytes()) for k in ("pitch", "energy", "mel_len")] == g[f"{case}_crc"].tolist()
    near = 0
    for b, n in enumerate(d["mel_len"].tolist()):
        for f, name in enumerate(("pitch", "energy")):
            v = d[name][b, :n].numpy().astype(np.float64)
            assert not d[name][b, n:].any()
            if n == 0 or np.isnan(v).any():
                assert g[f"{case}_kept"][b, f] == 0
                continue
            p25, p75, lower, upper = fr.bounds64(v)
            if p75 != p25:
                eps = 2.0 ** -20 * (abs(p25) + abs(p75))
                near += int((np.abs(v - lower) <= eps).sum() + (np.abs(v - upper) <= eps).sum())
            assert len(fr.kept64(v, name == "pitch")) == g[f"{case}_kept"][b, f], f"{case}[{b}] {name}"
    assert near == 0


def test_stats_case_shapes_and_quirks():
    d = synth.make_stats_case("voices")
    assert d["pitch"].shape == (64, 1723) and int(d["mel_len"].max()) == 1723
    hz = {float(np.float32(1) / np.float32(t) * np.float32(22050)) for t in range(27, 525)} | {0.0}
    assert set(np.unique(d["pitch"].numpy()).tolist()) <= hz
    assert (d["energy"].numpy()[d["energy"].numpy() != 0] > 0).all()
    for b, n in enumerate(d["mel_len"].tolist()):
        assert d["pitch"][b, n - 1] == 0
    g = np.load(os.path.join(ROOT, "tests", "golden", "dataset_stats.npz"))
    assert (g["mostly_unvoiced_kept"][:4, 0] == 0).all() and g["mostly_unvoiced_kept"][4, 0] > 0
    assert g["constant_kept"].tolist()[2] == [0, 0] and g["constant_kept"][0, 1] == 0 and g["constant_kept"][1, 0] == 0
    assert (g["single_frame_kept"][:2] == 0).all() and (g["empty_len_kept"][[0, 2]] == 0).all()
    assert g["nan_kept"][0, 0] == 0 and g["nan_kept"][1, 1] == 0 and g["nan_kept"][0, 1] > 0


def test_fixture_reference_values_agree_with_float64():
    """The reference's fp32 StandardScaler against a float64 two-pass over the kept values: 1e-4 relative (20 times the
    5.2e-6 measured on a 280k-value probe); min and max exactly."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "dataset_stats.npz"))
    for case in synth.STATS_CASES:
        d = synth.make_stats_case(case)
        for name in ("pitch", "energy"):
            cnt, mn, mx, mean, std = fr.pooled64(d[name].numpy(), d["mel_len"].tolist(), name == "pitch")
            ref = g[f"{case}_{name}"]
            assert cnt == g[f"{case}_kept"][:, 0 if name == "pitch" else 1].sum()
            assert ref[0] == mn and ref[1] == mx
            assert abs(ref[2] - mean) <= 1e-4 * abs(mean) and abs(ref[3] - std) <= 1e-4 * std, (case, name, ref, mean, std)


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    E_NULL, E_SHAPE, E_UNSUP = -1, -2, -4
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fail first
    ok = dict(B=2, C=1, S=640, S_out=294, o=320, n=147, width=14, T=27)

    def resample(audio=one, taps=one, tap_floats=None, ld_b=640, ld_c=0, ld_out=294, **kw):
        a = dict(ok, **kw)
        tf = a["n"] * a["T"] if tap_floats is None else tap_floats
        return lib.ispk_resample_f32(audio, ld_b, ld_c, one, taps, tf, one, one, ld_out, None, a["B"], a["C"], a["S"], a["S_out"],
                                     a["o"], a["n"], a["width"], a["T"], None)

    assert resample(audio=None) == E_NULL and b"null" in lib.ispk_last_error_string()
    assert resample(taps=None) == E_NULL
    assert resample(S_out=293) == E_SHAPE and b"ceil" in lib.ispk_last_error_string()
    assert resample(B=0) == E_SHAPE and resample(C=65) == E_SHAPE and resample(T=0) == E_SHAPE
    assert resample(ld_b=639) == E_SHAPE and resample(ld_out=293) == E_SHAPE
    assert resample(C=2, ld_c=639, ld_b=1280) == E_SHAPE
    assert resample(n=1000, T=13, width=7, o=1001, S_out=640) == E_UNSUP and b"12288" in lib.ispk_last_error_string()   # 13,000 taps
    assert resample(tap_floats=100) == E_UNSUP
    assert resample(o=9000, n=1, width=0, T=1, S=9000, ld_b=9000, S_out=1, ld_out=1) == E_UNSUP            # a block wider than the span

    def stats(pitch=one, state=one, B=2, M=512, ld=None):
        ld = M if ld is None else ld
        return lib.ispk_feature_stats_f64(pitch, ld, one, ld, one, one, state, B, M, 0, None)

    assert stats(state=None) == E_NULL and stats(pitch=None) == E_NULL
    assert stats(M=4097) == E_SHAPE and b"4096" in lib.ispk_last_error_string()
    assert stats(B=-1) == E_SHAPE and stats(ld=511) == E_SHAPE
    assert stats(B=0) == 0                                          # nothing to fold, no reset: a no-op


def test_python_argument_checks_without_gpu():
    rs = Resampler(48000, 22050)
    lens = torch.tensor([100, 50], dtype=torch.int64)
    with pytest.raises(ValueError, match="unit stride"):
        rs(torch.zeros(2, 200)[:, ::2], lens)
    with pytest.raises(ValueError, match="unit stride"):
        rs(torch.zeros(2, 100, dtype=torch.float64), lens)
    with pytest.raises(ValueError, match="audio_len"):
        rs(torch.zeros(2, 100), lens.int())
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        rs(torch.zeros(2, 100), lens)
    with pytest.raises(runtime.IspkError, match="GPU"):
        DatasetStats("cpu")
    with pytest.raises(ValueError, match="expects"):
        AudioFrontEnd(Resampler(48000, 24000), AcousticFeatures(sample_rate=22050))
    front = AudioFrontEnd(rs, AcousticFeatures(sample_rate=22050))
    assert front.pitch and front.energy
    with pytest.raises(ValueError, match="mono"):
        front(torch.zeros(2, 2, 100), lens)


def test_set_pitch_stats_and_stats_dict_round_trip():
    from isp_tts_amd import config
    from isp_tts_amd.data import DatasetStatsResult, FeatureStats
    feats = AcousticFeatures(sample_rate=22050)
    tables = feats.tables
    feats.set_pitch_stats(150.5, 40.25)
    assert (feats.pitch_mean, feats.pitch_std) == (150.5, 40.25) and feats.tables is tables
    with pytest.raises(ValueError):
        feats.set_pitch_stats(1.0, 0.0)
    res = DatasetStatsResult(FeatureStats(50.0, 400.0, 150.5, 40.25, 10), FeatureStats(0.1, 6.0, 3.0, 0.8, 12))
    d = res.to_dict()
    assert set(d) == {"pitch", "energy"} and set(d["pitch"]) == {"min", "max", "mean", "std"} and res.counts == {"pitch": 10, "energy": 12}
    f2 = AcousticFeatures.from_config(dict(config.ACOUSTIC_DATASET, stats=d))
    assert (f2.pitch_mean, f2.pitch_std) == (150.5, 40.25)
