"""CPU: audio conditioning's host side - the K-weighting coefficients against the BS.1770 table, the float64 reference meter
against the standard's 997 Hz sine, the meter table's matrix powers, and the argument checks of ispk_audio_measure_f64 /
ispk_audio_apply_f32 / ispk_pcm16 and of the Python face, which run before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import conditioning_reference as cr
from isp_tts_amd import runtime
from isp_tts_amd.data import (AcousticFeatures, AudioConditioner, AudioFrontEnd, Resampler, k_weighting, meter_table,
                              to_pcm16)


def test_k_weighting_at_48k_is_the_bs1770_table():
    (sb, sa), (hb, ha) = k_weighting(48000)
    t = cr.BS1770_48K
    for got, want in ((sb, t["shelf_b"]), (sa, t["shelf_a"]), (hb, t["highpass_b"]), (ha, t["highpass_a"])):
        assert got.dtype == np.float64 and np.abs(got - np.array(want)).max() <= 1e-12
    assert abs(sb[0] - 1.53512485958697) <= 1e-12 and abs(sa[1] + 1.69065929318241) <= 1e-12
    assert abs(ha[1] + 1.99004745483398) <= 1e-12


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000, 96000])
def test_k_weighting_equals_the_restatement(fs):
    for (b, a), (rb, ra) in zip(k_weighting(fs), cr.k_weighting(fs)):
        assert np.array_equal(b, rb) and np.array_equal(a, ra)


@pytest.mark.parametrize("fs,want", [(48000, -3.01027), (22050, -2.98095)])
def test_reference_meter_on_the_full_scale_997_hz_sine(fs, want):
    """BS.1770's calibration: a 0 dBFS 997 Hz sine in one channel reads -3.01 LKFS."""
    x = np.sin(2 * np.pi * 997.0 * np.arange(5 * fs) / fs)
    L = cr.loudness(x, fs)
    assert abs(L - want) <= 1e-5
    if fs == 48000:
        assert abs(L + 3.0103) <= 1e-3


def test_reference_gates_and_short_inputs():
    fs = 22050
    assert cr.loudness(np.zeros(3 * fs), fs) == -math.inf
    x = 0.1 * np.sin(2 * np.pi * 440.0 * np.arange(8820) / fs)
    assert len(cr.block_powers(x[:8819], fs)) == 0 and len(cr.block_powers(x, fs)) == 1
    assert cr.loudness(x[:8819], fs) == -math.inf and math.isfinite(cr.loudness(x, fs))
    assert cr.trim(np.zeros(5000)) == (0, 0) and cr.trim(np.zeros(0)) == (0, 0) and cr.trim(x, top_db=None) == (0, 8820)
    y = np.concatenate([np.zeros(3000), x, np.zeros(3000)])
    s, e = cr.trim(y)
    assert s % 256 == 0 and 3000 - 1024 < s <= 3000 and 3000 + 8820 <= e <= 3000 + 8820 + 1024
    assert cr.trim(y, pad_frames=100) == (0, len(y))
    assert cr.gain_for(-math.inf, 0.5) == 1.0 and cr.gain_for(-20.0, 0.0, None) == 1.0
    assert cr.gain_for(-43.0, 0.5) == pytest.approx(10 ** (-1 / 20) / 0.5)          # + 20 dB would clip: the cap
    assert cr.gain_for(-13.0, 0.5) == pytest.approx(10 ** -0.5)


@pytest.mark.parametrize("fs", [16000, 22050, 48000])
def test_meter_table_powers_carry_the_filter_state(fs):
    """The kernel's scan: running a chunk of 32 samples from zero state and adding A^32 times the entry state equals running
    it from the entry state; A^(32 2^k) are the squarings."""
    tab = meter_table(fs)
    assert tab.shape == (152,) and tab.dtype == np.float64
    (b, a), (_, d) = cr.k_weighting(fs)
    assert np.array_equal(tab[:7], [b[0], b[1], b[2], a[1], a[2], d[1], d[2]])
    P = [tab[8 + 16 * k:24 + 16 * k].reshape(4, 4) for k in range(9)]

    def run(s, xs):
        s = list(s)
        ys = []
        for x in xs:
            y1 = b[0] * x + s[0]
            y2 = y1 + s[2]
            s = [b[1] * x + s[1] - a[1] * y1, b[2] * x - a[2] * y1, -2.0 * y1 - d[1] * y2 + s[3], y1 - d[2] * y2]
            ys.append(y2)
        return np.array(s), np.array(ys)

    x = np.random.default_rng(fs).standard_normal(32 * 16)
    s_seq, y_seq = run(np.zeros(4), x)
    (sb, sa), (hb, ha) = cr.k_weighting(fs)
    y_ref = cr.biquad(hb, ha, cr.biquad(sb, sa, x))
    assert np.abs(y_seq - y_ref).max() <= 1e-11 * np.abs(y_ref).max()                # the state form is the cascade
    s = np.zeros(4)
    for c in range(16):
        s = P[0] @ s + run(np.zeros(4), x[32 * c:32 * c + 32])[0]
    assert np.abs(s - s_seq).max() <= 1e-11 * np.abs(s_seq).max()
    for k in range(8):
        assert np.abs(P[k] @ P[k] - P[k + 1]).max() <= 1e-12 * max(1.0, np.abs(P[k + 1]).max())


def test_constructor_value_errors():
    with pytest.raises(ValueError, match="100 ms"):
        AudioConditioner(22051)
    with pytest.raises(ValueError, match="100 ms"):
        AudioConditioner(11025)
    with pytest.raises(ValueError):
        AudioConditioner(0)
    with pytest.raises(NotImplementedError):
        AudioConditioner(4000)
    with pytest.raises(ValueError, match="top_db"):
        AudioConditioner(22050, top_db=-3.0)
    with pytest.raises(ValueError, match="peak_limit"):
        AudioConditioner(22050, peak_limit=0.0)
    with pytest.raises(ValueError, match="pad_frames"):
        AudioConditioner(22050, pad_frames=-1)
    with pytest.raises(ValueError, match="ref"):
        AudioConditioner(22050, ref="mean")
    with pytest.raises(ValueError, match="target_lufs"):
        AudioConditioner(22050, target_lufs=float("nan"))
    with pytest.raises(ValueError):
        k_weighting(-5)
    c = AudioConditioner(22050)
    assert (c.target_lufs, c.top_db, c.pad_frames, c.ref, c.trim_mode) == (-23.0, 60.0, 0, "max", 1)
    assert c.peak_limit == 10 ** (-1 / 20) and c.trim_threshold == 10.0 ** -6.0
    assert AudioConditioner(22050, top_db=None).trim_mode == 0 and AudioConditioner(22050, ref=1.0, top_db=40.0).trim_threshold == 1e-4
    assert AudioConditioner(22050, target_lufs=None).target_lufs is None


def test_python_argument_checks_and_cpu_tensors():
    c = AudioConditioner(22050)
    lens = torch.tensor([100, 50], dtype=torch.int64)
    with pytest.raises(ValueError, match="unit stride"):
        c(torch.zeros(2, 200)[:, ::2], lens)
    with pytest.raises(ValueError, match="unit stride"):
        c(torch.zeros(2, 100, dtype=torch.float64), lens)
    with pytest.raises(ValueError, match="unit stride"):
        c(torch.zeros(2, 2, 100), lens)
    with pytest.raises(ValueError, match="audio_len"):
        c(torch.zeros(2, 100), lens.int())
    with pytest.raises(ValueError, match="audio_len"):
        c(torch.zeros(2, 100), lens[:1])
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        c(torch.zeros(2, 100), lens)
    with pytest.raises(ValueError, match="unit stride"):
        to_pcm16(torch.zeros(2, 100, dtype=torch.float64), lens)
    with pytest.raises(ValueError, match="audio_len"):
        to_pcm16(torch.zeros(2, 100), lens.int())
    with pytest.raises(ValueError, match="seed"):
        to_pcm16(torch.zeros(2, 100), lens, dither=True, seed=-1)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        to_pcm16(torch.zeros(2, 100), lens)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.audio_apply(torch.zeros(2, 100), torch.zeros(2, 2, dtype=torch.int64), None)
    rs, feats = Resampler(48000, 22050), AcousticFeatures(sample_rate=22050)
    with pytest.raises(ValueError, match="conditioner"):
        AudioFrontEnd(rs, feats, conditioner=AudioConditioner(24000))
    front = AudioFrontEnd(rs, feats, conditioner=c)
    assert front.conditioner is c and AudioFrontEnd(rs, feats).conditioner is None


def test_workspace_size():
    assert runtime.audio_measure_workspace_floats(1, 8192, 22050) == 2 * (32 + 1041 + 4)
    assert runtime.audio_measure_workspace_floats(64, 131072, 22050) == 2 * 64 * (512 + 16 * 1041 + 60)
    assert runtime.audio_measure_workspace_floats(3, 0, 8000) == 2 * 3 * (1 + 1041 + 1)


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4
    one = ctypes.c_void_p(64)  # never dereferenced: the checks fail first
    need = runtime.audio_measure_workspace_floats(2, 10000, 22050)

    def measure(audio=one, table=one, table_doubles=152, ws=one, ws_floats=need, ld=10000, B=2, S=10000, fs=22050, trim_mode=1,
                thr=1e-6, pad=0, gain_mode=1, target=-23.0, limit=0.89):
        return lib.ispk_audio_measure_f64(audio, ld, one, table, table_doubles, one, one, one, one, ws, ws_floats, B, S, fs,
                                          trim_mode, thr, pad, gain_mode, target, limit, None)

    assert measure(audio=None) == E_NULL and b"null" in lib.ispk_last_error_string()
    assert measure(table=None) == E_NULL and measure(ws=None) == E_NULL
    assert measure(B=65536) == E_SHAPE and measure(B=-1) == E_SHAPE
    assert measure(S=(1 << 24) + 1, ld=1 << 25) == E_SHAPE and b"2^24" in lib.ispk_last_error_string()
    assert measure(ld=9999) == E_SHAPE and measure(table_doubles=151) == E_SHAPE
    assert measure(fs=22051) == E_SHAPE and b"100 ms" in lib.ispk_last_error_string()
    assert measure(fs=4000) == E_UNSUP and measure(fs=1000000) == E_UNSUP
    assert measure(trim_mode=3) == E_SHAPE and measure(pad=-1) == E_SHAPE and measure(thr=-1.0) == E_SHAPE
    assert measure(limit=0.0) == E_SHAPE and measure(target=float("nan")) == E_SHAPE
    assert measure(ws_floats=need - 1) == E_ALIGN and b"workspace" in lib.ispk_last_error_string()
    assert measure(ws=ctypes.c_void_p(68)) == E_ALIGN
    assert measure(B=0) == 0 and measure(B=0, audio=None) == 0                                  # a no-op

    def apply(audio=one, bounds=one, out=ctypes.c_void_p(1 << 30), ld=100, ld_out=100, B=2, S=100, S_out=100):
        return lib.ispk_audio_apply_f32(audio, ld, bounds, None, out, ld_out, None, B, S, S_out, None)

    assert apply(audio=None) == E_NULL and apply(bounds=None) == E_NULL and apply(out=None) == E_NULL
    assert apply(ld=99) == E_SHAPE and apply(ld_out=99) == E_SHAPE and apply(B=65536) == E_SHAPE
    assert apply(S=(1 << 24) + 1, ld=1 << 25) == E_SHAPE
    assert apply(out=one) == E_SHAPE and b"alias" in lib.ispk_last_error_string()
    assert apply(out=ctypes.c_void_p(64 + 4 * 150)) == E_SHAPE                                    # overlaps the second row
    assert apply(B=0) == 0

    def pcm(audio=one, lens=one, out=one, ld=100, ld_out=100, B=2, S=100):
        return lib.ispk_pcm16(audio, ld, lens, out, ld_out, B, S, 1, 7, None)

    assert pcm(audio=None) == E_NULL and pcm(lens=None) == E_NULL and pcm(out=None) == E_NULL
    assert pcm(ld=99) == E_SHAPE and pcm(ld_out=99) == E_SHAPE and pcm(B=65536) == E_SHAPE and pcm(S=-1) == E_SHAPE
    assert pcm(B=0) == 0 and pcm(S=0, ld=0, ld_out=0) == 0
