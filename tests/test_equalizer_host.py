"""The equalizer without a GPU: the band designs against their defining properties and against the reference's other derivation
(tests/equalizer_reference.py), the kernel's table, every ValueError, the argument errors of the C and Python entry points, and
the Synthesizer's new argument.

Tolerances.  The design properties hold to 1e-12 in float64 (a handful of roundings of 2^-53 on values of order one; the
gains used stay within +-12 dB).  The table's powers come from a chain of matrix products, the test's from the serial recurrence
on unit states: with the sections used here (pole radius <= 0.9996, powers bounded by 800) the two differ by far less than 1e-9
of the largest entry - as long as neither squares: squaring the nearly defective transition of a 5 Hz corner loses nine digits
(3e-7 of the entries of A^8192), which is what test_table is there to catch.  8,192 serial steps of the recurrence add 8192 * 2^-53 = 9e-13 of the
largest intermediate per step at worst: the same 1e-9 of the scale holds it with room."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import equalizer_reference as R
from isp_tts_amd import data, longform, runtime
from isp_tts_amd.data import (Equalizer, bandpass, deemphasis, equalizer_table, highpass, highshelf, lowpass, lowshelf, notch, peaking,
                              preemphasis)

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
RATES = [22050, 48000]
TOL = 1e-12


def mag(sos, f, rate):
    return float(np.abs(R.response(sos, [f], rate))[0])


# ------------------------------------------------------------------------------------------------ the designs
@pytest.mark.parametrize("rate", RATES)
def test_design_properties(rate):
    ny = rate / 2.0
    # (corners from 1 kHz up: 1 + a1 + a2 of rounded coefficients is 2 (1 - cos w0) / a0 with an absolute error of 2^-52, so the DC
    # gain of a low-pass holds to 2^-52 / (1 - cos w0) - 3e-14 at 1 kHz, but 2e-12 at 80 Hz and 48 kHz, whatever the code does)
    for f0 in (1000.0, 3000.0, 0.3 * rate):
        for q in (math.sqrt(0.5), 0.4, 3.0):
            lp, hp = Equalizer(rate, [lowpass(f0, q)]).sos, Equalizer(rate, [highpass(f0, q)]).sos
            assert abs(mag(lp, 0.0, rate) - 1.0) <= TOL and mag(lp, ny, rate) <= TOL and abs(mag(lp, f0, rate) - q) <= TOL * max(q, 1.0)
            assert abs(mag(hp, ny, rate) - 1.0) <= TOL and mag(hp, 0.0, rate) <= TOL and abs(mag(hp, f0, rate) - q) <= TOL * max(q, 1.0)
            assert abs(mag(Equalizer(rate, [bandpass(f0, q)]).sos, f0, rate) - 1.0) <= TOL
            assert mag(Equalizer(rate, [notch(f0, q)]).sos, f0, rate) <= TOL
            for g in (-12.0, -3.0, 6.0, 12.0):
                G, half = 10.0 ** (g / 20.0), 10.0 ** (g / 40.0)
                pk = Equalizer(rate, [peaking(f0, g, q)]).sos
                assert abs(mag(pk, f0, rate) - G) <= TOL * max(G, 1.0) and abs(mag(pk, 0.0, rate) - 1.0) <= TOL and abs(mag(pk, ny, rate) - 1.0) <= TOL
                ls = Equalizer(rate, [lowshelf(f0, g, q)]).sos
                assert abs(mag(ls, 0.0, rate) - G) <= TOL * max(G, 1.0) and abs(mag(ls, ny, rate) - 1.0) <= TOL and abs(mag(ls, f0, rate) - half) <= TOL * max(G, 1.0)
                hs = Equalizer(rate, [highshelf(f0, g, q)]).sos
                assert abs(mag(hs, ny, rate) - G) <= TOL * max(G, 1.0) and abs(mag(hs, 0.0, rate) - 1.0) <= TOL and abs(mag(hs, f0, rate) - half) <= TOL * max(G, 1.0)


@pytest.mark.parametrize("rate", RATES)
def test_designs_equal_the_references(rate):
    """The cookbook's closed forms against the bilinear transform of its analogue prototypes, and the defaults."""
    bands = [(highpass(120.0), dict(kind="highpass", freq=120.0)), (lowpass(7000.0, 1.3), dict(kind="lowpass", freq=7000.0, q=1.3)),
             (bandpass(1800.0, 0.6), dict(kind="bandpass", freq=1800.0, q=0.6)), (notch(50.0, 8.0), dict(kind="notch", freq=50.0, q=8.0)),
             (peaking(3000.0, 5.0), dict(kind="peaking", freq=3000.0, gain_db=5.0, q=1.0)),
             (lowshelf(200.0, -6.0), dict(kind="lowshelf", freq=200.0, gain_db=-6.0)),
             (highshelf(6000.0, 4.0, 0.9), dict(kind="highshelf", freq=6000.0, gain_db=4.0, q=0.9)),
             (preemphasis(), dict(kind="preemphasis")), (deemphasis(0.9), dict(kind="deemphasis", coef=0.9))]
    for band, kw in bands:
        got = Equalizer(rate, [band]).sos
        assert got.dtype == np.float64 and got.shape == (1, 5)
        assert np.abs(got[0] - R.design(rate=rate, **kw)).max() <= TOL, band
    assert Equalizer(rate, [preemphasis()]).sos.tolist() == [[1.0, -0.97, 0.0, 0.0, 0.0]]
    assert Equalizer(rate, [deemphasis()]).sos.tolist() == [[1.0, 0.0, 0.0, -0.97, 0.0]]
    eq = Equalizer(rate, [b for b, _ in bands[:8]])
    f = np.array([0.0, 30.0, 440.0, 5000.0, rate / 2.0])
    h = eq.response(f)
    assert h.dtype == np.complex128 and h.shape == (5,)
    assert np.abs(h - R.response(eq.sos, f, rate)).max() <= TOL * np.abs(h).max()
    assert highpass(80.0).q == lowpass(80.0).q == lowshelf(80.0, 1.0).q == highshelf(80.0, 1.0).q == math.sqrt(0.5)
    assert peaking(80.0, 1.0).q == 1.0


def test_sos_layouts():
    five = Equalizer(22050, [highpass(80.0), peaking(1000.0, 6.0)]).sos
    six = np.insert(five, 3, 1.0, axis=1) * np.array([[2.0], [0.5]])            # scipy's layout, a0 = 2 and 0.5
    assert np.array_equal(Equalizer(22050, sos=five).sos, five)
    assert np.abs(Equalizer(22050, sos=six).sos - five).max() <= 2.0 ** -52 * np.abs(five).max()
    assert Equalizer(22050, sos=five.tolist()).sections == 2


def test_preemphasis_then_deemphasis_restores_the_signal():
    x = np.random.default_rng(0).standard_normal((2, 4000)) + 0.5
    y, outs, _ = R.cascade(x, np.stack([R.design("preemphasis", 22050), R.design("deemphasis", 22050)]))
    # each sample: one rounding in the difference, one in the sum, and the sum feeds back with 0.97: 2^-52 / (1 - 0.97) of the scale
    assert np.abs(y - x).max() <= 2.0 ** -52 / 0.03 * np.abs(outs).max()
    assert np.abs(outs[0] - x).max() > 0.1


# ------------------------------------------------------------------------------------------------ the table
def _cascade8(rate=48000):
    return [highpass(5.0), highpass(20.0), lowshelf(150.0, 4.0), peaking(1000.0, 6.0, 2.0), notch(50.0, 10.0), peaking(3000.0, -5.0),
            highshelf(8000.0, -3.0), lowpass(0.45 * rate)]


@pytest.mark.parametrize("n", [1, 2, 8])
def test_table(n):
    eq = Equalizer(48000, _cascade8()[:n])
    t = eq.table.numpy()
    assert t.dtype == np.float64 and t.shape == (runtime.EQ_TABLE_DOUBLES(n),) == (40 * n + 4 * n * n,)
    assert np.array_equal(t, equalizer_table(eq.sos))
    head = t[:8 * n].reshape(n, 8)
    assert np.array_equal(head[:, :5], eq.sos) and not head[:, 5:].any()
    # every section's powers: 32 2^j zero samples through the reference from the two unit states (column i = the image of e_i)
    powers = t[8 * n:40 * n].reshape(n, 8, 2, 2)
    for k in range(n):
        for j in range(8):
            _, s0, s1 = R.section(np.zeros((2, runtime.EQ_CHUNK_SAMPLES << j)), eq.sos[k], [1.0, 0.0], [0.0, 1.0])
            want = np.stack([s0, s1])
            assert np.abs(powers[k, j] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (k, j)
        A = np.array([[-eq.sos[k, 3], 1.0], [-eq.sos[k, 4], 0.0]])
        assert np.abs(powers[k, 0] - np.linalg.matrix_power(A, 32)).max() <= 1e-9 * np.abs(powers[k, 0]).max()
    # the joint matrix: 8,192 zero samples through the reference from a random joint state
    J = t[40 * n:].reshape(2 * n, 2 * n)
    s = np.random.default_rng(5).standard_normal((3, 2 * n))
    _, outs, final = R.cascade(np.zeros((3, runtime.EQ_SEGMENT_SAMPLES)), eq.sos, state=s)
    scale = max(np.abs(s).max(), np.abs(outs).max(), np.abs(final).max())
    assert np.abs(final - s @ J.T).max() <= 1e-9 * scale
    assert np.abs(final).max() > 1e-3 * np.abs(s).max()                         # the 5 Hz pole still remembers: not a test of zeros
    for k in range(n):                                                         # block lower-triangular
        assert not J[2 * k:2 * k + 2, 2 * k + 2:].any()


def test_fir_tables_are_exactly_zero():
    for bands in ([preemphasis()], [preemphasis(), preemphasis(0.5)]):
        eq = Equalizer(22050, bands)
        assert not eq.table.numpy()[8 * eq.sections:].any()


# ------------------------------------------------------------------------------------------------ what is refused
def test_value_errors():
    ok = highpass(80.0)
    for kw, match in ((dict(bands=[]), "1 .. 8"), (dict(bands=[ok] * 9), "1 .. 8"), (dict(sos=np.zeros((0, 5))), "1 .. 8"),
                      (dict(sos=np.tile([1.0, 0, 0, 0, 0], (9, 1))), "1 .. 8"), (dict(), "exactly one"),
                      (dict(bands=[ok], sos=[[1.0, 0, 0, 0, 0]]), "exactly one"),
                      (dict(bands=[highpass(0.0)]), "frequency"), (dict(bands=[lowpass(11025.0)]), "frequency"),
                      (dict(bands=[peaking(-5.0, 3.0)]), "frequency"), (dict(bands=[notch(20000.0, 1.0)]), "frequency"),
                      (dict(bands=[highpass(80.0, 0.0)]), "q > 0"), (dict(bands=[bandpass(80.0, -1.0)]), "q > 0"),
                      (dict(bands=[peaking(80.0, float("nan"))]), "finite"), (dict(bands=[highpass(float("inf"))]), "finite"),
                      (dict(bands=[lowshelf(80.0, 3.0, float("nan"))]), "finite"), (dict(bands=[preemphasis(float("inf"))]), "finite"),
                      (dict(bands=["highpass"]), "a band is made by"),
                      (dict(sos=[[1.0, 0, 0, float("nan"), 0]]), "finite"), (dict(sos=[[1.0, 0, 0, 0.0, 1.0, 0, 0]]), "sos"),
                      (dict(sos=[[1.0, 0, 0, 0.0, 0.5, 0.1]]), "a0"),
                      (dict(bands=[deemphasis(1.0)]), "unstable"), (dict(bands=[deemphasis(-1.5)]), "unstable"),
                      (dict(sos=[[1.0, 0, 0, 0.0, 1.0]]), "unstable"), (dict(sos=[[1.0, 0, 0, 1.6, 0.5]]), "unstable"),
                      (dict(sos=[[1.0, 0, 0, 0.0, -1.0]]), "unstable")):
        with pytest.raises(ValueError, match=match):
            Equalizer(22050, **kw)
    with pytest.raises(ValueError, match="sample_rate"):
        Equalizer(0, [ok])
    assert Equalizer(22050, [deemphasis(0.999)]).sections == 1 and Equalizer(22050, [ok] * 8).sections == 8


def _eq_args(**kw):
    """(audio, ld_audio, audio_len, table, table_doubles, sections, out, ld_out, out_len, workspace, workspace_doubles, B, S, s)"""
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)       # never dereferenced: the checks come before any launch
    a = dict(audio=one, ld_audio=8, audio_len=one, table=one, table_doubles=44, sections=1, out=two, ld_out=8, out_len=one,
             workspace=one, workspace_doubles=4, B=2, S=8, stream=None)
    a.update(kw)
    return list(a.values())


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    eq = lib.ispk_equalize_f32
    assert lib.ispk_equalize_segment_samples() == runtime.EQ_SEGMENT_SAMPLES == 8192
    assert runtime.SIGNATURES["ispk_equalize_f32"] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                       ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    assert runtime.ABI_VERSION == 2
    for name in ("audio", "audio_len", "table", "out", "workspace"):
        assert eq(*_eq_args(**{name: None})) == E_NULL, name
        assert b"null" in lib.ispk_last_error_string()
    for n in (0, -1, 9):
        assert eq(*_eq_args(sections=n, table_doubles=runtime.EQ_TABLE_DOUBLES(max(n, 0)))) == E_SHAPE, n
        assert b"sections" in lib.ispk_last_error_string()
    assert eq(*_eq_args(table_doubles=45)) == E_SHAPE and b"table" in lib.ispk_last_error_string()
    assert eq(*_eq_args(sections=8, table_doubles=44)) == E_SHAPE
    assert eq(*_eq_args(B=65536)) == E_SHAPE
    assert eq(*_eq_args(S=(1 << 24) + 1, ld_audio=1 << 25, ld_out=1 << 25)) == E_SHAPE and b"2^24" in lib.ispk_last_error_string()
    assert eq(*_eq_args(S=-1)) == E_SHAPE
    assert eq(*_eq_args(ld_audio=7)) == E_SHAPE
    assert eq(*_eq_args(ld_out=7)) == E_SHAPE and b"strides" in lib.ispk_last_error_string()
    assert eq(*_eq_args(workspace_doubles=3)) == E_ALIGN and b"workspace" in lib.ispk_last_error_string()
    assert eq(*_eq_args(workspace=ctypes.c_void_p(20))) == E_ALIGN
    assert eq(*_eq_args(S=8193, ld_audio=8200, ld_out=8200, workspace_doubles=7)) == E_ALIGN      # two segments: 2 * 2 * 2 doubles
    # out overlapping audio without being audio
    assert eq(*_eq_args(out=ctypes.c_void_p(16 + 4))) == E_SHAPE and b"overlaps" in lib.ispk_last_error_string()
    assert eq(*_eq_args(out=ctypes.c_void_p(16 + 4 * 15))) == E_SHAPE                             # the last sample of audio
    assert eq(*_eq_args(out=ctypes.c_void_p(16), ld_out=12)) == E_SHAPE                           # the same base, another stride
    # B = 0 returns before the pointers are looked at; the scalars are checked first
    assert eq(*_eq_args(B=0, audio=None, out=None)) == 0
    assert eq(*_eq_args(B=0, sections=9)) == E_SHAPE


def test_python_face():
    from isp_tts_amd.bindings import audio
    names = {"equalize", "EQ_MAX_SECTIONS", "EQ_SEGMENT_SAMPLES", "EQ_TABLE_DOUBLES", "equalize_workspace_doubles"}
    assert names <= set(audio.__all__) and names <= set(runtime.__dict__)
    assert runtime.EQ_MAX_SECTIONS == 8 and runtime.EQ_TABLE_DOUBLES(8) == 576
    assert runtime.equalize_workspace_doubles(3, 8192, 2) == 12 and runtime.equalize_workspace_doubles(3, 8193, 2) == 24
    assert runtime.equalize_workspace_doubles(3, 0, 1) == 6
    for name in ("Equalizer", "highpass", "lowpass", "bandpass", "notch", "peaking", "lowshelf", "highshelf", "preemphasis", "deemphasis"):
        assert hasattr(data, name), name
    eq = Equalizer(22050, [highpass(80.0)])
    a, n = torch.zeros((2, 64)), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        eq(a, n)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.equalize(a, n, eq.table, 1)
    with pytest.raises(ValueError, match="audio"):
        eq(a.double(), n)
    with pytest.raises(ValueError, match="audio_len"):
        eq(a, n.int())
    o = eq.empty_outputs(2, 20000, "cpu")
    assert set(o) == {"audio", "audio_len", "work"} and o["work"].dtype == torch.float64 and o["work"].numel() == 2 * 3 * 2
    assert inspect.signature(longform.Synthesizer).parameters["equalizer"].default is None
