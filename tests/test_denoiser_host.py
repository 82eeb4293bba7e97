"""CPU: the denoiser's float64 reference (tests/denoiser_reference.py) against torch.stft / shrink / torch.istft, the argument
checks of ispk_denoise_f32, which run before any launch, and the Denoiser module's construction, state dict and refusals."""
import ctypes

import numpy as np
import pytest
import torch

import denoiser_reference as dr
from isp_tts_amd import runtime
from isp_tts_amd.acoustic.evaluator import SynthesisEvaluator
from isp_tts_amd.denoiser import Denoiser, denoise_tables, frame0_magnitude, hann_window

E_NULL, E_SHAPE = -1, -2


def _torch_chain(x: np.ndarray, bias: np.ndarray, strength: float) -> np.ndarray:
    n = x.shape[0]
    w = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    X = torch.stft(torch.from_numpy(x), 1024, hop_length=256, win_length=1024, window=w, center=True, pad_mode="reflect",
                   return_complex=True)                                          # [513, F]
    mag = X.abs()
    t = strength * torch.from_numpy(bias)[:, None]
    Y = torch.where(mag > 0, X * torch.clamp(1 - t / mag, min=0), torch.zeros_like(X))
    return torch.istft(Y, 1024, hop_length=256, win_length=1024, window=w, center=True, length=n).numpy()


@pytest.mark.parametrize("n", [513, 768, 769, 4097, 20000])
def test_reference_is_torch_stft_shrink_istft(n):
    x = dr.make_signal(n, seed=n)
    assert np.array_equal(hann_window(), dr.window())
    assert float(np.abs(dr.window() - torch.hann_window(1024, periodic=True, dtype=torch.float64).numpy()).max()) <= 1e-15
    X = dr.stft(x)
    assert X.shape == (1 + n // 256, 513)
    bias = np.median(np.abs(X), axis=0)
    want = _torch_chain(x, bias, 1.0)
    got = dr.denoise(x, bias, 1.0)
    peak = float(np.abs(want).max())
    assert peak > 0.05 and 0.3 <= dr.zeroed_share(x, bias, 1.0) <= 0.7        # the clamp acts on both sides
    assert float(np.abs(got - want).max()) <= 1e-12 * peak
    assert float(np.abs(got - x).max()) > 1e-3                                   # the shrink did something
    back = dr.denoise(x, bias, 0.0)
    assert float(np.abs(back - x).max()) <= 1e-12
    assert float(np.abs(_torch_chain(x, bias, 0.0) - x).max()) <= 1e-12


@pytest.mark.parametrize("n", [0, 1, 512])
def test_reference_copies_short_utterances(n):
    x = dr.make_signal(n, seed=7)
    got = dr.denoise(x, np.ones(513), 5.0)
    assert got.shape == (n,) and np.array_equal(got, x) and got is not x
    batch = dr.denoise_batch(np.stack([np.pad(x, (0, 600 - n))] * 2), [n, 601], np.ones(513), 5.0)
    assert np.array_equal(batch[0, :n], x) and not batch[0, n:].any() and not batch[1].any()      # 601 > S counts as 0


def test_frame0_magnitude_is_the_reference_frame():
    x = dr.make_signal(2052, seed=3)
    assert float(np.abs(frame0_magnitude(x) - np.abs(dr.stft(x)[0])).max()) <= 1e-12
    with pytest.raises(ValueError, match="at least 513"):
        frame0_magnitude(x[:512])
    t = denoise_tables()
    assert t.dtype == torch.float32 and t.shape == (runtime.DENOISE_TABLE_FLOATS,)
    assert np.array_equal(t[4096:].numpy(), dr.window().astype(np.float32))
    a = 2.0 * np.pi * np.arange(2048) / 2048.0
    assert np.array_equal(t[:4096].numpy().reshape(2048, 2), np.stack([np.cos(a), -np.sin(a)], 1).astype(np.float32))


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    ts = lib.ispk_denoise_tile_samples()
    assert ts > 0 and ts % 256 == 0 and ts == runtime.DENOISE_TILE_SAMPLES
    assert (runtime.DENOISE_N_FFT, runtime.DENOISE_HOP) == (1024, 256)
    one, other = ctypes.c_void_p(16), ctypes.c_void_p(4096)      # never dereferenced: the checks fail first
    err = lambda: lib.ispk_last_error_string()
    fn = lib.ispk_denoise_f32
    args = lambda **kw: tuple({**dict(audio=one, ld_audio=1000, audio_len=None, tables=one, bias=one, strength_item=None,
                                      strength=0.5, out=other, ld_out=1000, B=2, S=1000, stream=None), **kw}.values())
    for name in ("audio", "tables", "bias", "out"):
        assert fn(*args(**{name: None})) == E_NULL and b"null" in err(), name
    assert fn(*args(ld_audio=999)) == E_SHAPE and b"row strides" in err()
    assert fn(*args(ld_out=999)) == E_SHAPE and b"row strides" in err()
    assert fn(*args(B=65536)) == E_SHAPE and b"shape" in err()
    assert fn(*args(S=2 ** 31 - 1, ld_audio=2 ** 31, ld_out=2 ** 31)) == E_SHAPE and b"shape" in err()
    assert fn(*args(out=one)) == E_SHAPE and b"may not be audio" in err()                # neighbours read the halo
    assert fn(*args(strength=-0.25)) == E_SHAPE and b"negative" in err()
    assert fn(*args(strength=float("nan"))) == E_SHAPE and b"NaN" in err()
    assert fn(*args(B=0, audio=None)) == 0 and fn(*args(S=0, ld_audio=0, ld_out=0, out=None)) == 0   # zero-sized: no-ops
    # scalar loads and stores: rows need no alignment, so there is no E_ALIGN rule to check


def test_module_buffer_and_state_dict():
    bias = torch.rand(513, generator=torch.Generator().manual_seed(0)).double()
    for shaped in (bias, bias[:, None], bias[None, :, None]):
        d = Denoiser(shaped)
        assert list(d.state_dict()) == ["bias_spec"]
        assert d.bias_spec.shape == (1, 513, 1) and d.bias_spec.dtype == torch.float32
        assert torch.equal(d.bias_spec.flatten(), bias.float()) and d.strength == 0.01
    d = Denoiser(torch.zeros(513), strength=0.1)
    published = {"bias_spec": bias.float().reshape(1, 513, 1)}
    d.load_state_dict(published, strict=True)
    assert torch.equal(d.bias_spec, published["bias_spec"])
    d.load_state_dict(dict(published, **{"stft.forward_basis": torch.zeros(1026, 1, 1024)}), strict=True)   # conv bases: ignored
    assert Denoiser(bias, filter_length=1024, hop_length=256, win_length=1024, n_overlap=4).strength == 0.01


def test_module_refusals():
    ok = torch.ones(513)
    for bad in (-ok, ok * float("nan"), ok * float("inf"), torch.cat([ok[:-1], torch.tensor([-1e-9])])):
        with pytest.raises(ValueError, match="finite and >= 0"):
            Denoiser(bad)
    for shape in ((512,), (1, 513), (513, 2), (2, 513, 1)):
        with pytest.raises(ValueError, match="bias_spec"):
            Denoiser(torch.ones(shape))
    for kw, word in ((dict(filter_length=2048), "filter_length 2048"), (dict(hop_length=512), "hop_length 512"),
                     (dict(win_length=800), "win_length 800"), (dict(n_overlap=8), "n_overlap 8")):
        with pytest.raises(NotImplementedError, match=word):
            Denoiser(ok, **kw)
    with pytest.raises(ValueError, match="negative or NaN"):
        Denoiser(ok, strength=-1.0)
    d = Denoiser(ok)
    with pytest.raises(runtime.IspkError, match="GPU"):
        d(torch.zeros(2, 1000), torch.tensor([1000, 900]))
    with pytest.raises(runtime.IspkError, match="GPU"):
        runtime.denoise(torch.zeros(2, 1000), None, denoise_tables(), ok, 0.5)
    with pytest.raises(ValueError, match="mode"):
        Denoiser.from_vocoder(None, mode="ones")


def test_score_infer_denoiser_needs_a_vocoder():
    ev = SynthesisEvaluator.__new__(SynthesisEvaluator)          # the check runs before anything of the evaluator is used
    with pytest.raises(ValueError, match="denoiser needs the vocoder"):
        ev.score_infer(None, {}, denoiser=Denoiser(torch.ones(513)))
