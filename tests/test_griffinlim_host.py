"""CPU: the Griffin-Lim float64 reference (tests/griffinlim_reference.py) against torch.stft / torch.istft, against the
reference providers' mel (tests/golden/features.npz: the framing is the extractor's), its fixed point, its convergence, the hash
mirror, the argument checks of the two entry points, which run before any launch, and the GriffinLim module's construction.

torch.istft refuses center=False with a Hann window (the envelope at padded position 0 is w[0]^2 = 0), so the overlap-add is
compared with torch.istft(center=True) of the same frames, which returns padded positions 512 .. = samples 128 .. n; the first
128 samples are covered by the fixed-point test (a consistent pair returns x to 1e-12 everywhere).

Reference figures (float64, hashed start, seed 0): spectral convergence after 0 / 32 / 64 iterations harmonic 0.630 / 0.181 /
0.124, chirp 0.603 / 0.147 / 0.126, noise 0.626 / 0.174 / 0.142; worst ratio of consecutive values 0.9949 / 0.9987 / 0.9956.  Mel
round trip, mean |log-mel difference| after 32 iterations over that after 0: harmonic 0.262, noise 0.101."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import griffinlim_reference as gr
from conftest import ROOT
from isp_tts_amd import config, runtime, synth
from isp_tts_amd.data import AcousticFeatures
from isp_tts_amd.denoiser import denoise_tables
from isp_tts_amd.griffinlim import GriffinLim, filterbank_pinv

E_NULL, E_SHAPE, E_UNSUP = -1, -2, -4
CLIPS = (("harmonic", 8192), ("chirp", 12032), ("noise", 4096))


def _clip(kind, n):
    return synth.make_clip(kind, n, 0.5).double().numpy()


@pytest.mark.parametrize("kind,n", CLIPS + (("noise", 256), ("harmonic", 768)))
def test_reference_is_torch_stft_and_istft(kind, n):
    x = _clip(kind, n)
    T = n // 256
    w = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    assert float(np.abs(gr.window() - w.numpy()).max()) <= 1e-15
    xp = torch.from_numpy(gr.pad(x))
    X = torch.stft(xp, 1024, hop_length=256, win_length=1024, window=w, center=False, return_complex=True)      # [513, T]
    got = gr.stft(x)
    assert got.shape == (T, 513) == tuple(X.shape[::-1])
    assert float(np.abs(got - X.numpy().T).max()) <= 1e-12 * float(np.abs(got).max())
    # overlap-add of a spectrum that is not consistent: the clip's magnitude with hashed phases
    Y = np.abs(got) * np.exp(2j * np.pi * gr.hashed_phase(5, T))
    Y[:, 0], Y[:, -1] = Y[:, 0].real, Y[:, -1].real
    mine = gr.istft(Y)
    want = torch.istft(torch.from_numpy(Y.T.copy()), 1024, hop_length=256, win_length=1024, window=w, center=True,
                       length=n - 128).numpy()
    peak = float(np.abs(mine).max())
    assert mine.shape == (n,) and peak > 1e-3
    assert float(np.abs(mine[128:] - want).max()) <= 1e-12 * peak


@pytest.mark.parametrize("case", list(synth.FEATURE_CASES))
def test_reference_framing_is_the_extractors(case):
    """magnitude -> filterbank -> log of the reference equals the reference providers' mel, within the extractor tests' fp32
    bounds (tests/test_gpu_features.py: log-mel within 1e-4 where the float64 mel is >= 1e-2 of its frame's largest, linear mel
    within 2e-6 of the frame's largest elsewhere)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "features.npz"))
    waves = synth.make_feature_case(case)
    assert [zlib.crc32(w.numpy().tobytes()) for w in waves] == g[f"{case}_crc"].tolist(), "synth clips changed"
    fb = AcousticFeatures.from_config(config.ACOUSTIC_DATASET).fb.double().numpy()
    checked = 0
    for b, wave in enumerate(waves):
        x = wave.double().numpy()
        T = len(x) // 256
        assert g[f"{case}_mel_len"][b] == T
        lin64 = (np.abs(gr.stft(x)) @ fb).T                                        # [80, T]
        want = g[f"{case}_mel"][b, :, :T].astype(np.float64)
        fmax = np.maximum(lin64.max(0), 1e-30)
        big = lin64 >= 1e-2 * fmax
        err = np.abs(gr.log_mel(x, fb) - want)
        assert (err[big] <= 1e-4).all(), f"{case}[{b}]: log-mel error {err[big].max():.2e}"
        small = np.abs(np.maximum(lin64, 1e-5) - np.exp(want))
        assert (small[~big] <= 2e-6 * np.broadcast_to(fmax, lin64.shape)[~big] + 1e-9).all(), f"{case}[{b}]: small mel"
        checked += int(big.sum())
    assert checked > 500


@pytest.mark.parametrize("kind,n", CLIPS + (("noise", 256), ("harmonic", 512)))
def test_one_step_is_the_identity_on_a_consistent_pair(kind, n):
    x = _clip(kind, n)
    back = gr.step(x, np.abs(gr.stft(x)))
    assert float(np.abs(back - x).max()) <= 1e-12
    assert gr.spectral_convergence(x, np.abs(gr.stft(x))) <= 1e-12


@pytest.fixture(scope="module")
def runs():
    """kind -> (M, the 65 waveforms of 64 iterations from the hashed phase), made once."""
    out = {}
    for kind, n in CLIPS:
        M = np.abs(gr.stft(_clip(kind, n)))
        out[kind] = (M, gr.griffinlim(M, 64, seed=0, keep=range(65)))
    return out


@pytest.mark.parametrize("kind", [k for k, _ in CLIPS])
def test_spectral_convergence_falls_at_every_iteration(runs, kind):
    M, xs = runs[kind]
    sc = np.array([gr.spectral_convergence(xs[i], M) for i in range(65)])
    ratio = sc[1:] / sc[:-1]
    print(f"{kind}: spectral convergence {sc[0]:.4f} -> {sc[32]:.4f} -> {sc[64]:.4f}, worst ratio {ratio.max():.4f}")
    assert (ratio < 0.999).all(), f"{kind}: ratio {ratio.max():.5f} at iteration {int(ratio.argmax()) + 1}"
    assert sc[0] > 0.3 and sc[64] < 0.2


@pytest.mark.parametrize("kind,n,measured", [("harmonic", 8192, 0.262), ("noise", 4096, 0.101)])
def test_mel_round_trip_of_the_reference(kind, n, measured):
    fb = AcousticFeatures().fb.double().numpy()
    x = _clip(kind, n)
    mel = gr.log_mel(x, fb)
    ys = gr.griffinlim(gr.mel_to_linear(mel, gr.pinv(fb)), 32, seed=0, keep=(0, 32))
    d0, d32 = (float(np.abs(gr.log_mel(ys[i], fb) - mel).mean()) for i in (0, 32))
    print(f"{kind}: mean |log-mel difference| {d0:.4f} -> {d32:.4f}, ratio {d32 / d0:.3f}")
    assert d32 < 0.5 * d0
    assert abs(d32 / d0 - measured) <= 0.01                                   # the docstring's figure


def test_hash_mirror():
    """mix_seed is the splitmix64 finaliser (its first output for state 0 is the published 0xE220A8397B1DCDAF); drop_hash is
    one lowbias32 round over (idx ^ low word) xor the high word, restated here in Python integers."""
    assert gr.mix_seed(0) == 0xE220A8397B1DCDAF and gr.mix_seed(1) == 0x910A2DEC89025CC1

    def lowbias32(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    known = {0: (0x6E062EDC, 0x75DFD289, 0x942CC473, 0x7411074D), 1: (0x7D761EFC, 0x08390182, 0x3637B359, 0x26182B3C),
             2 ** 64 - 1: (0xEC2F394C, 0x08A44583, 0xAB684BDC, 0x5DD709FA)}
    idx = (0, 1, 513, 2 ** 32 - 1)
    for seed, want in known.items():
        word = gr.mix_seed(seed)
        assert tuple(lowbias32(i ^ (word & 0xFFFFFFFF)) ^ (word >> 32) for i in idx) == want
        assert tuple(int(v) for v in gr.drop_hash(word, np.array(idx, dtype=np.uint32))) == want
    u = gr.hashed_phase(0, 3)
    assert u.shape == (3, 513) and u.min() >= 0 and u.max() < 1
    assert u[0, 0] == (0x6E062EDC >> 8) * 2.0 ** -24 and u[1, 0] == (0x942CC473 >> 8) * 2.0 ** -24      # index 513 f + k
    assert np.array_equal(gr.hashed_phase(0, 2), u[:2])                      # a function of (seed, f, k) only
    assert abs(float(u.mean()) - 0.5) < 0.03 and not np.array_equal(gr.hashed_phase(1, 3), u)


def test_pseudo_inverse():
    fb = AcousticFeatures().fb.double().numpy()
    P = gr.pinv(fb)
    assert P.shape == (513, 80) and np.array_equal(P, filterbank_pinv(fb))
    A = fb.T                                                                 # mel = A magnitude
    assert float(np.abs(A @ P @ A - A).max()) <= 1e-12 and float(np.abs(P @ A @ P - P).max()) <= 1e-9 * float(np.abs(P).max())
    assert float(np.abs(A @ P - np.eye(80)).max()) <= 1e-10                  # full row rank: a right inverse
    gl = GriffinLim()
    assert gl.pinv_t.shape == (80, 513) and gl.pinv_t.dtype == torch.float32
    assert np.array_equal(gl.pinv_t.numpy(), P.T.astype(np.float32))         # float64, rounded once
    assert gl.tables.shape == (runtime.DENOISE_TABLE_FLOATS,) and torch.equal(gl.tables, denoise_tables())
    assert list(gl.state_dict()) == []                                       # tables, not state
    feats = AcousticFeatures(sample_rate=16000, n_mels=64, f_max=None)
    g2 = GriffinLim.from_features(feats, n_iter=8, seed=3)
    assert (g2.sample_rate, g2.n_mels, g2.n_iter, g2.seed, g2.hop_length) == (16000, 64, 8, 3, 256)
    assert np.array_equal(g2.pinv_t.numpy(), gr.pinv(feats.fb.double().numpy()).T.astype(np.float32))
    assert torch.equal(GriffinLim(sample_rate=16000, n_mels=64, f_max=None).pinv_t, g2.pinv_t)
    mel = np.log(np.maximum(fb.T @ np.abs(gr.stft(_clip("harmonic", 2048))).T, 1e-5))
    M = gr.mel_to_linear(mel, P)
    assert M.shape == (8, 513) and M.min() == 0.0 and (M == 0).any() and M.max() > 1.0     # the clamp acts


def test_constructor_refusals():
    for kw, word in ((dict(n_fft=2048), "n_fft 2048"), (dict(hop_length=512), "hop_length 512"),
                     (dict(win_length=800), "win_length 800"), (dict(window="hamming"), "window 'hamming'"),
                     (dict(momentum=0.99), "momentum 0.99"), (dict(mel_scale="htk"), "mel_scale 'htk'"),
                     (dict(norm=None), "norm None"), (dict(n_mels=129), "n_mels=129"), (dict(n_mels=0), "n_mels=0")):
        with pytest.raises(NotImplementedError, match=word):
            GriffinLim(**kw)
    for kw in (dict(n_iter=-1), dict(n_iter=1.5), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError, match="n_iter|seed"):
            GriffinLim(**kw)
    gl = GriffinLim(n_fft=1024, hop_length=256, win_length=1024, window="hann", momentum=0.0)
    assert gl.n_iter == 32 and gl.seed == 0
    with pytest.raises(runtime.IspkError, match="GPU"):
        gl(torch.zeros(2, 80, 4))
    with pytest.raises(runtime.IspkError, match="GPU"):
        gl.magnitude(torch.zeros(2, 80, 4), torch.tensor([4, 3]))
    with pytest.raises(runtime.IspkError, match="GPU"):
        gl.from_magnitude(torch.zeros(2, 4, 513))
    with pytest.raises(runtime.IspkError, match="GPU"):
        runtime.mel_to_linear(torch.zeros(2, 80, 4), None, gl.pinv_t)
    with pytest.raises(runtime.IspkError, match="GPU"):
        runtime.griffinlim_step(None, torch.zeros(2, 4, 513), None, gl.tables, torch.zeros(2, 1024), mode=runtime.GRIFFINLIM_INIT)


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    ts = lib.ispk_griffinlim_tile_samples()
    assert ts == 4096 == runtime.GRIFFINLIM_TILE_SAMPLES
    assert (runtime.GRIFFINLIM_N_FFT, runtime.GRIFFINLIM_HOP, runtime.GRIFFINLIM_PAD) == (1024, 256, 384)
    assert (runtime.GRIFFINLIM_STEP, runtime.GRIFFINLIM_INIT) == (0, 1)
    one, other = ctypes.c_void_p(16), ctypes.c_void_p(4096)      # never dereferenced: the checks fail first
    err = lambda: lib.ispk_last_error_string()
    fn = lib.ispk_griffinlim_step_f32
    args = lambda **kw: tuple({**dict(audio=one, ld_audio=1024, mag=one, ld_mag=4 * 513, mel_len=None, tables=one, out=other,
                                      ld_out=1024, audio_len=None, B=2, T=4, mode=0, seed=0, stream=None), **kw}.values())
    for name in ("audio", "mag", "tables", "out"):
        assert fn(*args(**{name: None})) == E_NULL and b"null" in err(), name
    assert fn(*args(ld_audio=1023)) == E_SHAPE and b"row strides" in err()
    assert fn(*args(ld_out=1023)) == E_SHAPE and b"row strides" in err()
    assert fn(*args(ld_mag=4 * 513 - 1)) == E_SHAPE and b"row strides" in err()
    assert fn(*args(B=65536)) == E_SHAPE and b"shape" in err()
    assert fn(*args(T=8388576, ld_audio=2 ** 31, ld_out=2 ** 31, ld_mag=2 ** 33)) == E_SHAPE and b"shape" in err()
    assert fn(*args(out=one)) == E_SHAPE and b"may not be audio" in err()                # neighbours read the halo
    assert fn(*args(mode=2)) == E_UNSUP and b"mode" in err()
    assert fn(*args(mode=1, audio=None, ld_audio=0, out=None)) == E_NULL                 # init reads no audio, still needs out
    assert fn(*args(B=0, audio=None)) == 0 and fn(*args(T=0, ld_audio=0, ld_out=0, ld_mag=0, out=None)) == 0   # no-ops
    fn = lib.ispk_mel_to_linear_f32
    args = lambda **kw: tuple({**dict(mel=one, mel_f16=0, sb=320, sc=4, st=1, mel_len=None, pinv_t=one, mag=other,
                                      ld_mag=4 * 513, B=2, n_mels=80, T=4, stream=None), **kw}.values())
    for name in ("mel", "pinv_t", "mag"):
        assert fn(*args(**{name: None})) == E_NULL and b"null" in err(), name
    assert fn(*args(n_mels=129)) == E_SHAPE and fn(*args(n_mels=0)) == E_SHAPE and b"shape" in err()
    assert fn(*args(B=65536)) == E_SHAPE and fn(*args(T=8388576, ld_mag=2 ** 33)) == E_SHAPE
    assert fn(*args(ld_mag=4 * 513 - 1)) == E_SHAPE and b"leading stride" in err()
    assert fn(*args(B=0, mel=None)) == 0 and fn(*args(T=0, mag=None, ld_mag=0)) == 0
