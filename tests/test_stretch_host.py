"""CPU: the time stretch's float64 reference (tests/stretch_reference.py) against itself - the textbook recurrence equals its
modulo-2-pi form, rate 1 returns the input, the integer arithmetic equals torch.arange's and Python's round - the condition that
the GPU tests' bound rests on (8 x the mixed chain's error stays under 2e-4 on the named inputs), the argument validation of
data.TimeStretch / data.PitchShift, and the C entry's argument errors, none of which touches a GPU."""
import ctypes
import math

import pytest
import torch

import stretch_reference as R
from isp_tts_amd import runtime
from isp_tts_amd.data import PitchShift, TimeStretch, nearest_ratio

RATES = (0.5, 0.8, 1.0, 1.25, 1.37, 2.0)
LENGTHS = (513, 1024, 4095, 4096, 4097, 8191, 12288)


@pytest.mark.parametrize("r", (0.5, 0.8, 1.37, 2.0))
def test_textbook_equals_modulo_form(r):
    for n, seed in ((5000, 2), (12288, 3)):
        x = R.signal(n, seed)
        a, b = R.stretch_item(x, r, "textbook"), R.stretch_item(x, r, "modulo")
        assert len(a) == len(b) == round(n / r)
        assert R.relative_error(b, a) <= 1e-9, (n, r)


def test_rate_one_returns_the_input():
    for n, seed in ((513, 1), (4097, 2), (12288, 3)):
        x = R.signal(n, seed)
        y = R.stretch_item(x, 1.0)
        assert len(y) == n and R.plan(n, 1.0) == (1 + n // 256, 1 + n // 256, n)
        assert R.relative_error(y, x) <= 1e-9, n


def test_integers():
    for n in LENGTHS + (5119, 777, 100000):
        for r in RATES:
            F, Fo, wanted = R.plan(n, r)
            assert F == 1 + n // 256
            assert Fo == torch.arange(0, F, r, dtype=torch.float64).numel(), (n, r)
            assert wanted == round(n / r), (n, r)
            i, a = R.frame_times(Fo, r)
            assert i[0] == 0 and i[-1] <= F - 1 and (0.0 <= a).all() and (a < 1.0).all()
            assert Fo == 0 or (Fo - 1) * r < F <= Fo * r
            assert 256 * (Fo - 1) + 512 >= wanted, "every sample below wanted lies under an output frame"
    assert R.plan(5119, 1.25) == (20, 16, 4095)                            # F / r an exact integer
    assert R.plan(4096, 0.5)[2] == 8192 and round(513 / 2.0) == 256        # 256.5 rounds to even
    assert R.lengths(512, 1.0, 600) == (512, 512, R.SHORT) and R.lengths(0, 1.0, 600) == (0, 0, R.SHORT)
    assert R.lengths(1024, 0.5, 2000) == (2000, 2048, R.TRUNCATED)
    assert R.lengths(1024, 3.0, 600) == (600, 1024, R.BAD_RATE | R.TRUNCATED)
    assert R.lengths(1024, float("nan"), 2000) == (1024, 1024, R.BAD_RATE)


def test_mixed_chain_condition_on_the_named_inputs():
    """8 x e_mixed <= 2e-4 for the inputs of the GPU tests: shown with the reference alone."""
    worst = 0.0
    for n in (513, 4097, 12288):
        for k, r in enumerate(RATES):
            x = R.signal(n, 100 * n + k)
            e = R.relative_error(R.mixed_item(x, r), R.stretch_item(x, r))
            worst = max(worst, e)
            assert 0.0 < 8.0 * e <= 2e-4, (n, r, e)
    print(f"mixed chain: worst error / peak {worst:.2e}")
    assert worst <= 1.25e-5


def test_tone_with_noise_keeps_its_peak_in_the_reference():
    n = 12288
    x = R.tone_signal(n, 5)
    for r in (0.8, 1.25):
        y = R.stretch_item(x, r)
        assert len(y) == round(n / r) and R.peak_bin(y) == R.peak_bin(x) == round(440.0 * 8192 / R.RATE_HZ)


def test_time_stretch_validation():
    for bad in (0.49, 2.01, float("nan"), "1.0", True):
        with pytest.raises(ValueError, match="rate"):
            TimeStretch(bad)
    ts = TimeStretch()
    assert ts.rate is None and TimeStretch(1.25).rate == 1.25 and TimeStretch(2).rate == 2.0
    assert ts.tables.dtype == torch.float32 and ts.tables.shape == (5120,)
    assert TimeStretch.out_samples(4096, 0.8) == 5121 and TimeStretch.out_samples(4097, 2.0) == 2050
    audio, n = torch.zeros(2, 1024), torch.tensor([1024, 600])
    with pytest.raises(ValueError, match="no rate"):
        ts(audio, n)
    with pytest.raises(ValueError, match="rate"):
        ts(audio, n, rate=2.5)
    with pytest.raises(ValueError, match="audio_len"):
        ts(audio, n.int(), rate=1.0)
    with pytest.raises(ValueError, match="audio"):
        ts(audio.double(), n, rate=1.0)
    with pytest.raises(ValueError, match="audio"):
        ts(audio[:, ::2], n, rate=1.0)
    with pytest.raises(ValueError, match="rate"):
        ts(audio, n, rate=torch.ones(2))                                   # fp32
    with pytest.raises(ValueError, match="rate"):
        ts(audio, n, rate=torch.ones(3, dtype=torch.float64))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        ts(audio, n, rate=1.0)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        ts(audio, n, rate=torch.ones(2, dtype=torch.float64), out_samples=2048)
    with pytest.raises(ValueError, match="samples"):
        ts.empty_outputs(2, "cpu", samples=0)
    out = ts.empty_outputs(2, "cpu", samples=2049)
    assert out["audio"].shape == (2, 2049) and out["work"].numel() == runtime.stretch_workspace_bytes(2, 0, 2049) == 8 * 2 * 1 * 1026
    assert runtime.stretch_workspace_bytes(3, 100, 4097) == 8 * 3 * 2 * 1026
    rows = ts.manifest({"audio_len": torch.tensor([2000, 512]), "wanted": torch.tensor([2048, 512]), "flags": torch.tensor([2, 5])},
                       ["a", "b"], torch.tensor([1024, 512]))
    assert rows == [{"name": "a", "samples_in": 1024, "samples_out": 2000, "wanted": 2048, "flags": ("truncated",)},
                    {"name": "b", "samples_in": 512, "samples_out": 512, "wanted": 512, "flags": ("short", "bad_rate")}]
    with pytest.raises(ValueError, match="names"):
        ts.manifest({"audio_len": torch.tensor([1]), "wanted": torch.tensor([1]), "flags": torch.tensor([0])}, [])


def test_pitch_shift_validation():
    ps = PitchShift(22050, steps=1)
    assert ps.ratio == (18, 17) and ps.stretch.rate == 17 / 18 and (ps.resampler.o, ps.resampler.n) == (18, 17)
    assert ps.cents_error == pytest.approx(1200.0 * math.log2((18 / 17) / 2.0 ** (1 / 12))) and -1.1 < ps.cents_error < -1.0
    assert PitchShift(22050, steps=-12).ratio == (1, 2) and PitchShift(22050, steps=12).ratio == (2, 1)
    assert PitchShift(22050, steps=0).ratio == (1, 1) and PitchShift(22050, steps=7).ratio == (3, 2)
    assert PitchShift(22050, ratio=(10, 8)).ratio == (5, 4) and PitchShift(22050, ratio=(5, 4)).cents_error == 0.0
    assert nearest_ratio(2.0 ** (1 / 12), 8) == (1, 1) and nearest_ratio(1.5, 32) == (3, 2) and nearest_ratio(0.66, 3) == (2, 3)
    assert ps.stretched_samples(1700) == 1801
    for kw in (dict(), dict(steps=1, ratio=(5, 4)), dict(steps=float("inf")), dict(ratio=(5, 0)), dict(ratio=(5.5, 4)), dict(ratio=(5,)),
               dict(steps=13), dict(ratio=(1, 3)), dict(steps=1, max_den=0)):
        with pytest.raises(ValueError):
            PitchShift(22050, **kw)
    with pytest.raises(ValueError, match="sample_rate"):
        PitchShift(0, steps=1)
    with pytest.raises(NotImplementedError):
        PitchShift(22050, ratio=(2003, 1999))                              # more phases than the resampler's table holds
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        ps(torch.zeros(1, 1024), torch.tensor([1024]))


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    assert lib.ispk_stretch_tile_samples() == runtime.STRETCH_TILE_SAMPLES == 4096
    size = ctypes.c_int64(-1)
    assert lib.ispk_stretch_workspace_bytes(3, 100, 4097, ctypes.byref(size)) == 0 and size.value == runtime.stretch_workspace_bytes(3, 100, 4097)
    assert lib.ispk_stretch_workspace_bytes(1, 1, 0, ctypes.byref(size)) == 0 and size.value == runtime.stretch_workspace_bytes(1, 1, 0)
    assert lib.ispk_stretch_workspace_bytes(1, 1, 1, None) == E_NULL
    assert lib.ispk_stretch_workspace_bytes(65536, 1, 1, ctypes.byref(size)) == E_SHAPE
    assert lib.ispk_stretch_workspace_bytes(1, 1, (1 << 24) + 1, ctypes.byref(size)) == E_SHAPE
    one, off = ctypes.c_void_p(16), ctypes.c_void_p(20)      # never dereferenced: every check fails before a launch
    other = ctypes.c_void_p(32)
    need = runtime.stretch_workspace_bytes(2, 1024, 1500)

    def call(audio=one, ld=1024, n=one, tables=one, rate=1.0, rates=None, out=other, ldo=1500, osamp=1500, olen=one, wanted=one,
             flags=one, ws=one, wsb=need, B=2, S=1024):
        return lib.ispk_stretch_f32(audio, ld, n, tables, rate, rates, out, ldo, osamp, olen, wanted, flags, ws, wsb, B, S, None)

    for kw in (dict(audio=None), dict(n=None), dict(tables=None), dict(out=None), dict(olen=None), dict(wanted=None), dict(flags=None),
               dict(ws=None)):
        assert call(**kw) == E_NULL, kw
        assert b"null" in lib.ispk_last_error_string()
    for kw in (dict(B=65536), dict(S=(1 << 24) + 1, ld=1 << 25), dict(S=0), dict(osamp=(1 << 24) + 1, ldo=1 << 25), dict(osamp=0),
               dict(ld=1023), dict(ldo=1499), dict(out=one), dict(B=-1)):
        assert call(**kw) == E_SHAPE, kw
    for rate in (0.49, 2.5, float("nan"), -1.0):
        assert call(rate=rate) == E_SHAPE, rate
        assert b"[0.5, 2]" in lib.ispk_last_error_string()
    assert call(wsb=need - 1) == E_ALIGN and b"workspace" in lib.ispk_last_error_string()
    assert call(ws=off) == E_ALIGN
    assert call(B=0) == 0 and call(B=0, audio=None, out=None) == 0          # a no-op
