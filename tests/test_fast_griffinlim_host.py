"""CPU: the fast (momentum) Griffin-Lim float64 reference (tests/fast_griffinlim_reference.py): its two forms - the textbook
loop that keeps the complex tprev, and the plain step applied to x_n - a x_{n-1} that the kernel computes - agree; its spectral
convergence figures; its first iterations; FastGriffinLim's construction; and the argument checks of
ispk_griffinlim_fast_step_f32 and ispk_griffinlim_error_f32, which run before any launch.

Reference figures (float64, magnitude rounded to fp32, hashed start, seed 0, 32 iterations), spectral convergence plain /
momentum 0.99 / momentum 0.5: harmonic 8192 0.1808 / 0.0484 / 0.1482, chirp 12032 0.1471 / 0.0645 / 0.1270, noise 4096 0.1740 /
0.1051 / 0.1447.  The two forms differ by at most 3.2e-12 of the peak after 32 iterations.  At momentum 0.99 the figure is not
monotone (it rises once on harmonic and twice on chirp), so only its value after 32 iterations is held."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fast_griffinlim_reference as fr
import griffinlim_reference as gr
from isp_tts_amd import runtime, synth
from isp_tts_amd.data import AcousticFeatures
from isp_tts_amd.griffinlim import FastGriffinLim, GriffinLim

E_NULL, E_SHAPE = -1, -2
CLIPS = (("harmonic", 8192), ("chirp", 12032), ("noise", 4096))
MOMENTA = (0.99, 0.5)
TABLE = {"harmonic": (0.1808, 0.0484, 0.1482), "chirp": (0.1471, 0.0645, 0.1270), "noise": (0.1740, 0.1051, 0.1447)}


@pytest.fixture(scope="module")
def runs():
    """kind -> (M rounded to fp32, plain {0, 1, 2, 32}, {momentum: (textbook {1, 2, 32}, waveform difference {1, 2, 32})})."""
    out = {}
    for kind, n in CLIPS:
        M = np.abs(gr.stft(synth.make_clip(kind, n, 0.5).double().numpy())).astype(np.float32).astype(np.float64)
        fast = {m: (fr.textbook(M, 32, m, keep=(1, 2, 32)), fr.waveform_difference(M, 32, m, keep=(1, 2, 32))) for m in MOMENTA}
        out[kind] = (M, gr.griffinlim(M, 32, seed=0, keep=(0, 1, 2, 32)), fast)
    return out


@pytest.mark.parametrize("kind", [k for k, _ in CLIPS])
@pytest.mark.parametrize("momentum", MOMENTA)
def test_the_two_forms_agree(runs, kind, momentum):
    _, _, fast = runs[kind]
    book, diff = fast[momentum]
    peak = float(np.abs(book[32]).max())
    err = float(np.abs(book[32] - diff[32]).max())
    print(f"{kind} momentum {momentum}: textbook against waveform difference after 32 iterations {err / peak:.1e} of the peak")
    assert peak > 1e-3 and err <= 1e-9 * peak


@pytest.mark.parametrize("kind", [k for k, _ in CLIPS])
def test_spectral_convergence_table(runs, kind):
    M, plain, fast = runs[kind]
    sc_plain = gr.spectral_convergence(plain[32], M)
    sc = {m: gr.spectral_convergence(fast[m][0][32], M) for m in MOMENTA}
    print(f"{kind}: plain {sc_plain:.4f}, momentum 0.99 {sc[0.99]:.4f} (ratio {sc[0.99] / sc_plain:.2f}), 0.5 {sc[0.5]:.4f}")
    for got, want in zip((sc_plain, sc[0.99], sc[0.5]), TABLE[kind]):
        assert abs(got - want) <= 0.002, (kind, got, want)
    assert sc[0.99] <= 0.75 * sc_plain


@pytest.mark.parametrize("kind", [k for k, _ in CLIPS])
@pytest.mark.parametrize("momentum", MOMENTA)
def test_first_iterations(runs, kind, momentum):
    """x_{-1} = 0: iteration 1 is the plain step exactly.  Iteration 2 already differs: at the default momentum 0.99 (a = 0.497)
    by more than 0.05 of the plain iterate's peak (harmonic 0.178, chirp 0.067, noise 0.059).  At momentum 0.5 (a = 0.333) the
    difference is smaller (0.158, 0.038, 0.038) and is held to 0.01, a hundred times the GPU tests' bound of 1e-4 of the peak
    against this reference: that bound cannot pass with the momentum left out."""
    _, plain, fast = runs[kind]
    for form in fast[momentum]:
        assert np.array_equal(form[1], plain[1])
        d = float(np.abs(form[2] - plain[2]).max()) / float(np.abs(plain[2]).max())
        print(f"{kind} momentum {momentum}: iteration 2 differs from the plain one by {d:.3f} of the peak")
        assert d > (0.05 if momentum == 0.99 else 0.01)


def test_init_is_the_start(runs):
    M, plain, fast = runs["noise"]
    for f in (fr.textbook, fr.waveform_difference):
        assert np.array_equal(f(M, 2, 0.99, init=plain[0]), fast[0.99][0 if f is fr.textbook else 1][2])
        assert np.array_equal(f(M, 0, 0.99, seed=0), plain[0])


def test_constructor():
    for m in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            FastGriffinLim(momentum=m)
    gl = FastGriffinLim()
    assert gl.momentum == 0.99 and gl.n_iter == 32 and gl.seed == 0 and isinstance(gl, GriffinLim)
    assert FastGriffinLim(momentum=0).momentum == 0.0 and FastGriffinLim(momentum=0.5, n_iter=4).momentum == 0.5
    assert list(gl.state_dict()) == []
    assert torch.equal(gl.pinv_t, GriffinLim().pinv_t) and torch.equal(gl.tables, GriffinLim().tables)
    feats = AcousticFeatures(sample_rate=16000, n_mels=64, f_max=None)
    g2 = FastGriffinLim.from_features(feats, n_iter=8, seed=3, momentum=0.5)
    assert (g2.sample_rate, g2.n_mels, g2.n_iter, g2.seed, g2.momentum) == (16000, 64, 8, 3, 0.5)
    assert FastGriffinLim.from_features(feats).momentum == 0.99
    assert torch.equal(g2.pinv_t, GriffinLim.from_features(feats).pinv_t)
    with pytest.raises(NotImplementedError, match="FastGriffinLim"):           # the plain class points to the fast one
        GriffinLim(momentum=0.99)
    with pytest.raises(NotImplementedError, match="n_fft 2048"):
        FastGriffinLim(n_fft=2048)
    with pytest.raises(ValueError, match="momentum"):
        gl.from_magnitude(torch.zeros(2, 4, 513), momentum=1.5)
    for call in (lambda: gl(torch.zeros(2, 80, 4)), lambda: gl.from_magnitude(torch.zeros(2, 4, 513)),
                 lambda: gl.spectral_convergence(torch.zeros(2, 1024), torch.zeros(2, 4, 513)),
                 lambda: runtime.griffinlim_fast_step(torch.zeros(2, 1024), torch.zeros(2, 1024), 0.5, torch.zeros(2, 4, 513),
                                                      None, gl.tables, torch.zeros(2, 1024)),
                 lambda: runtime.griffinlim_error(torch.zeros(2, 1024), torch.zeros(2, 4, 513), None, gl.tables)):
        with pytest.raises(runtime.IspkError, match="GPU"):
            call()


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    one, other, third = ctypes.c_void_p(16), ctypes.c_void_p(4096), ctypes.c_void_p(8192)      # never dereferenced
    err = lambda: lib.ispk_last_error_string()
    fn = lib.ispk_griffinlim_fast_step_f32
    args = lambda **kw: tuple({**dict(audio=one, ld_audio=1024, prev=other, ld_prev=1024, alpha=0.5, mag=one, ld_mag=4 * 513,
                                      mel_len=None, tables=one, out=third, ld_out=1024, audio_len=None, B=2, T=4, stream=None),
                               **kw}.values())
    for name in ("audio", "prev", "mag", "tables", "out"):
        assert fn(*args(**{name: None})) == E_NULL and b"null" in err(), name
    for name in ("ld_audio", "ld_prev", "ld_out"):
        assert fn(*args(**{name: 1023})) == E_SHAPE and b"row strides" in err(), name
    assert fn(*args(ld_mag=4 * 513 - 1)) == E_SHAPE and b"row strides" in err()
    assert fn(*args(B=65536)) == E_SHAPE and b"shape" in err()
    big = dict(T=8388576, ld_audio=2 ** 31, ld_prev=2 ** 31, ld_out=2 ** 31, ld_mag=2 ** 33)
    assert fn(*args(**big)) == E_SHAPE and b"shape" in err()
    assert fn(*args(out=one)) == E_SHAPE and b"may not be audio or prev" in err()        # neighbours read the halo
    assert fn(*args(out=other)) == E_SHAPE and b"may not be audio or prev" in err()
    for alpha in (1.0, -0.1, 1.5, math.nan, math.inf):
        assert fn(*args(alpha=alpha)) == E_SHAPE and b"alpha" in err(), alpha
    assert fn(*args(B=0, audio=None, prev=None)) == 0                                    # no-ops
    assert fn(*args(T=0, ld_audio=0, ld_prev=0, ld_out=0, ld_mag=0, out=None)) == 0
    fn = lib.ispk_griffinlim_error_f32
    args = lambda **kw: tuple({**dict(audio=one, ld_audio=1024, mag=one, ld_mag=4 * 513, mel_len=None, tables=one, work=other,
                                      ld_work=8, err=third, B=2, T=4, stream=None), **kw}.values())
    for name in ("audio", "mag", "tables", "work", "err"):
        assert fn(*args(**{name: None})) == E_NULL and b"null" in err(), name
    for name, short in (("ld_audio", 1023), ("ld_mag", 4 * 513 - 1), ("ld_work", 7)):
        assert fn(*args(**{name: short})) == E_SHAPE and b"row strides" in err(), name
    assert fn(*args(B=65536)) == E_SHAPE and b"shape" in err()
    assert fn(*args(T=8388576, ld_audio=2 ** 31, ld_mag=2 ** 33, ld_work=2 ** 25)) == E_SHAPE and b"shape" in err()
    assert fn(*args(B=0, audio=None, err=None)) == 0                                     # no-ops
    assert fn(*args(T=0, ld_audio=0, ld_mag=0, ld_work=0, work=None)) == 0
