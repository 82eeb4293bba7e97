"""CPU: the host side of the pitch tracker (isp_tts_amd.data.pitch) and its float64 reference (tests/pyin_reference.py): the
public names, from_config's pitch.method, the table builders against the reference's own formulas, the reference on a steady tone,
the reference in fp32 against itself in float64 on the GPU tests' clip, and the entries' argument checks without a GPU."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import pyin_reference as R
from isp_tts_amd import config, runtime
from isp_tts_amd.data import AcousticFeatures
from isp_tts_amd.data import pitch as P

SR = 22050


def test_public_names():
    from isp_tts_amd.data import PitchTracker
    t = PitchTracker(SR)
    assert (t.n_bins, t.width, t.min_period, t.max_period) == (481, 51, 25, 401)
    assert t.prior.dtype == torch.float64 and t.prior.shape == (runtime.PYIN_TABLE_DOUBLES,)
    assert t.trans.shape == (51 + 481 + 3,)
    n = t.normalised(166.6, 62.5)
    assert n is not t and (n.mean, n.std) == (166.6, 62.5) and t.mean is None and n.prior is t.prior and n._on is t._on
    with pytest.raises(ValueError):
        t.normalised(1.0, 0.0)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        t(torch.zeros(1, 512), torch.tensor([512]))
    for bad in (dict(f_min=0.0), dict(f_min=900.0), dict(bins_per_semitone=0), dict(switch_prob=1.0)):
        with pytest.raises(ValueError):
            PitchTracker(SR, **bad)
    with pytest.raises(NotImplementedError, match="bins"):
        PitchTracker(SR, f_min=20.0, f_max=10000.0)
    with pytest.raises(NotImplementedError, match="window"):
        PitchTracker(8000)


def test_from_config_accepts_pyin_and_still_refuses_penn():
    d = copy.deepcopy(config.ACOUSTIC_DATASET)
    default = AcousticFeatures.from_config(d)
    assert default.pitch_method == "torch-yin" and default.tracker is None
    d["pitch"]["method"] = "pyin"
    f = AcousticFeatures.from_config(d)
    assert f.pitch_method == "pyin" and f.tracker is not None and f.tracker.f_min == 40.0      # the recipe's pitch.f_min
    assert (f.tracker.n_bins, f.tracker.max_period) == (519, 552)
    del d["pitch"]["f_min"]
    assert AcousticFeatures.from_config(d).tracker.f_min == 55.0
    assert f.tracker.f_max == float(d["pitch"].get("f_max", 800)) and (f.pitch_mean, f.pitch_std) == (default.pitch_mean, default.pitch_std)
    assert torch.equal(f.tables, default.tables) and torch.equal(f.fb_index, default.fb_index)
    d["pitch"]["f_min"] = 65.0
    assert AcousticFeatures.from_config(d).tracker.f_min == 65.0
    d["pitch"]["method"] = "penn"
    with pytest.raises(NotImplementedError, match="pitch method 'penn': only torch-yin is built"):
        AcousticFeatures.from_config(d)
    with pytest.raises(NotImplementedError, match="only torch-yin is built"):
        AcousticFeatures(pitch_method="crepe")


def test_tables_match_the_reference_formulas():
    prior = P.beta_prior()
    assert prior.shape == (100,) and (prior >= 0).all() and (prior[:50] > 0).all() and abs(prior.sum() - 1.0) <= 1e-15
    thr, want = R.thresholds_and_prior()
    tab = P.observation_table().numpy()
    assert np.array_equal(tab[:100], thr) and np.array_equal(tab[100:200], want) and np.array_equal(tab[100:200], prior)
    assert tab[200] == 0.0 and np.array_equal(tab[201:301], np.cumsum(prior)) and abs(tab[300] - 1.0) <= 1e-15
    k = np.arange(512)
    assert np.allclose(tab[301:813], (1 - np.exp(-2.0)) * np.exp(-2.0 * k), rtol=1e-15, atol=0)
    assert tab[813] == 0.0 and np.allclose(tab[814:], 1.0 / (1.0 - np.exp(-2.0 * np.arange(1, 513))), rtol=1e-15, atol=0)
    # the closed form of I_x(2, 18): both sides are about twenty float64 roundings of values below 1 (eps = 2.2e-16)
    x = np.linspace(0, 1, 101)
    assert np.abs(P.beta_cdf(x, 2, 18) - (1 - (1 - x) ** 19 - 19 * x * (1 - x) ** 18)).max() <= 20 * 2.3e-16
    assert P.pitch_bins(55.0, 880.0) == R.n_bins(55.0, 880.0) == 481
    assert P.transition_width(SR) == R.width_of(SR) == 51
    assert P.pitch_periods(SR, 55.0, 880.0) == R.periods(SR, 55.0, 880.0) == (25, 401)
    for nb, width in ((481, 51), (33, 7), (130, 21), (5, 11)):
        got = P.transition_table(nb, width).numpy()
        logtri, lognorm, ls, lw, li = R.transition_tables(nb, width)
        assert np.array_equal(got[:width], logtri) and np.allclose(got[width:width + nb], lognorm, rtol=0, atol=1e-15)
        assert (got[width + nb], got[width + nb + 1], got[width + nb + 2]) == (ls, lw, li)
        # the tables stand for a stochastic matrix: every row of exp(logtri - lognorm + stay | switch) sums to 1
        dense = R.transition_matrix(nb, width)
        assert np.abs(dense.sum(axis=1) - 1.0).max() <= 1e-14
        h = (width - 1) // 2
        for i in (0, nb // 2, nb - 1):
            row = np.zeros(2 * nb)
            for kk in range(width):
                j = i + kk - h
                if 0 <= j < nb:
                    row[j] = np.exp(got[kk] - got[width + i] + ls)
                    row[nb + j] = np.exp(got[kk] - got[width + i] + lw)
            assert np.abs(row - dense[i]).max() <= 1e-14 and abs(row.sum() - 1.0) <= 1e-14


def test_workspace_and_shapes():
    assert runtime.pyin_workspace_bytes(3, 78, 481) == 16 * 3 * 78 + (2 * 3 * 78 * 481 + 7) // 8 * 8
    lib = runtime.lib()
    n = ctypes.c_int64(0)
    assert lib.ispk_pyin_workspace_bytes(3, 78, 481, ctypes.byref(n)) == 0 and n.value == runtime.pyin_workspace_bytes(3, 78, 481)
    assert lib.ispk_pyin_workspace_bytes(1, 1, 33, ctypes.byref(n)) == 0 and n.value == 16 + 72 == runtime.pyin_workspace_bytes(1, 1, 33)
    assert lib.ispk_pyin_frames_per_block() == runtime.PYIN_FRAMES_PER_BLOCK
    t = P.PitchTracker(SR)
    out = t.empty_outputs(2, 20000)
    assert out["obs"].shape == (2, 78, 481) and out["f0"].shape == (2, 78) and "pitch" not in out
    assert out["work"].numel() == runtime.pyin_workspace_bytes(2, 78, 481)
    assert t.normalised(0.0, 1.0).empty_outputs(2, 20000)["pitch"].shape == (2, 78)


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    one = ctypes.c_void_p(16)
    obs = lambda *a: lib.ispk_pyin_observe_f32(*a, None)       # noqa: E731
    assert obs(None, 512, one, one, one, one, None, 1, 512, 2, 481, 25, 401, 22050.0, 55.0, 10) == E_NULL
    assert obs(one, 512, one, one, one, one, None, 1, 512, 0, 481, 25, 401, 22050.0, 55.0, 10) == E_SHAPE     # M below the frames of S
    assert obs(one, 512, one, one, one, one, None, 1, 512, 2, 1025, 25, 401, 22050.0, 55.0, 10) == E_SHAPE
    assert obs(one, 512, one, one, one, one, None, 1, 512, 2, 481, 25, 1023, 22050.0, 55.0, 10) == E_SHAPE
    assert obs(one, 512, one, one, one, one, None, 1, 512, 2, 481, 25, 26, 22050.0, 55.0, 10) == E_SHAPE
    assert obs(one, 100, one, one, one, one, None, 1, 512, 2, 481, 25, 401, 22050.0, 55.0, 10) == E_SHAPE
    assert obs(one, 512, one, one, one, one, None, 0, 512, 2, 481, 25, 401, 22050.0, 55.0, 10) == 0
    dec = lambda *a: lib.ispk_pyin_decode_f64(*a, None)        # noqa: E731
    tail = (one, one, one, one, None, None, one)
    assert dec(one, 0, None, one, 50, 55.0, 10, 0.0, 1.0, *tail, one, 1 << 20, 1, 4, 33) == E_SHAPE            # an even width
    assert dec(one, 0, None, one, 129, 55.0, 10, 0.0, 1.0, *tail, one, 1 << 20, 1, 4, 33) == E_SHAPE
    assert b"byte" in lib.ispk_last_error_string()
    assert dec(one, 0, None, one, 7, 55.0, 10, 0.0, 1.0, *tail, one, 1 << 20, 1, 4, 1025) == E_SHAPE
    assert dec(one, 0, None, one, 7, 55.0, 10, 0.0, 0.0, one, one, one, one, one, None, one, one, 1 << 20, 1, 4, 33) == E_SHAPE   # std 0
    assert dec(None, 0, None, one, 7, 55.0, 10, 0.0, 1.0, *tail, one, 1 << 20, 1, 4, 33) == E_NULL
    assert dec(one, 0, None, one, 7, 55.0, 10, 0.0, 1.0, *tail, one, runtime.pyin_workspace_bytes(1, 4, 33) - 1, 1, 4, 33) == E_ALIGN
    assert dec(one, 0, None, one, 7, 55.0, 10, 0.0, 1.0, *tail, ctypes.c_void_p(20), 1 << 20, 1, 4, 33) == E_ALIGN
    assert dec(one, 0, None, one, 7, 55.0, 10, 0.0, 1.0, *tail, one, 1 << 20, 0, 4, 33) == 0


def test_reference_tracks_a_steady_tone_to_its_bin():
    """A steady 220 Hz tone of five harmonics: 220 = 55 * 2^2 is bin 240 exactly; every frame whose window lies inside the tone is
    voiced at that bin, and the path's re-scored log-probability is the decoder's own."""
    t = np.arange(8192) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * 220.0 * h * t) / h for h in range(1, 6))
    f0, voiced, states, logp, rows = R.track(x, SR)
    assert len(f0) == R.frames_of(8192) == 32
    inner = slice(2, 26)                     # windows [256 t - 384, 256 t + 1664) inside [0, 8192)
    assert voiced[inner].all() and (states[inner] == 240).all() and np.abs(f0[inner] - 220.0).max() < 1e-9
    assert rows[inner, 240].min() > 0.5
    nb, width = 481, 51
    logobs, _ = R.log_observations(rows)
    again = R.path_log_prob(states, logobs, R.transition_tables(nb, width), width)
    assert abs(again - logp) <= 1e-9 * abs(logp)


def test_viterbi_against_a_dense_recursion():
    """The banded block-maximum recursion equals a dense Viterbi over the full transition matrix where no tie occurs (random
    continuous scores), and resolves planted ties to the lowest state index."""
    g = np.random.default_rng(3)
    nb, width = 12, 5
    tables = R.transition_tables(nb, width)
    logobs = np.log(g.uniform(0.05, 1.0, (9, 2 * nb)))
    states, logp = R.viterbi(logobs, tables, width)
    with np.errstate(divide="ignore"):
        lt = np.log(R.transition_matrix(nb, width))
    delta = tables[4] + logobs[0]
    back = []
    for t in range(1, len(logobs)):
        cand = delta[:, None] + lt
        back.append(cand.argmax(axis=0))
        delta = cand.max(axis=0) + logobs[t]
    s = int(delta.argmax())
    want = [s]
    for b in reversed(back):
        s = int(b[s])
        want.append(s)
    assert list(states) == want[::-1] and abs(logp - delta.max()) <= 1e-12 * abs(logp)
    # all-equal observations: every path within the band ties; the first maximum at every step walks to state 0's neighbourhood
    flat = np.zeros((4, 2 * nb))
    exact = (np.zeros(width), np.zeros(nb), 0.0, 0.0, 0.0)
    states, logp = R.viterbi(flat, exact, width)
    assert logp == 0.0 and states[-1] == 0 and (states == 0).all()


def test_fp32_difference_function_gives_the_same_rows_on_the_clip():
    """The GPU test's clip: the restatement with its difference function carried out in fp32 gives the float64 rows on (nearly)
    every frame, so the GPU test's 5 % cap on excluded frames has room.  The 42 frames whose 2,048 samples lie inside one of the
    two stretches of tone are voiced in any case.  The clip's margins (the float64 distances from a decision point) are printed."""
    x = R.clip()
    assert R.frames_of(len(x)) == 78
    rows64, margins = R.observe_item(x, SR)
    rows32, _ = R.observe_item(x, SR, dtype=np.float32)
    differing = int((np.abs(rows64 - rows32).max(axis=1) > 1e-6).sum())
    voiced = int((rows64.sum(axis=1) > 0.5).sum())
    print(f"clip: {differing} of 78 frames differ between fp32 and float64 difference functions; {voiced} voiced")
    m_thr = sorted(m["threshold"] for m in margins)[:3]
    m_nb = sorted(m["neighbour"] for m in margins)[:3]
    print(f"smallest trough-to-threshold distances {m_thr}, neighbour distances {m_nb}")
    assert differing <= 1 and voiced >= 42
