"""Vocoder denoiser: removes a generator's constant "bias" spectrum from its waveforms, the stage the FastPitch-family HiFi-GAN
inference scripts apply to every synthesised utterance.

The bias is the magnitude spectrum of what the generator emits for an empty mel (its hum and checkpoint-specific tones).  Per
utterance x[0, n), n >= 513, with N = 1024, hop 256, K = 513 bins and w the periodic Hann window:

    xp[p]  = x[r(p - 512)], p < n + 1024;  r(i) = -i below 0, 2 (n - 1) - i from n on, else i           (reflect padding)
    X_f[k] = sum_j xp[256 f + j] w[j] exp(-2 pi i j k / 1024),  f < F = 1 + n // 256
    Y_f[k] = X_f[k] max(1 - strength bias[k] / |X_f[k]|, 0)        (= max(|X| - strength bias, 0) with the phase kept)
    y_f    = irfft(Y_f)
    out[s] = sum_f w[j] y_f[j] / sum_f w[j]^2,  j = s + 512 - 256 f, over the utterance's own frames; 0 from n on

which is what torch.stft(center=True, pad_mode="reflect"), the shrink and torch.istft(center=True, length=n) compute, and what
the conv-basis STFT of the FastPitch-family `Denoiser` computes.  Utterances below 513 samples (where the reflection is
undefined and torch refuses) come back unchanged.  The whole of it is one launch of ispk_denoise_f32 (csrc/denoise.hip): no
ATen compute, no host read, one stream, capturable with out=, and an utterance's samples do not depend on its batch.

    denoiser = Denoiser.from_vocoder(vocoder)                 # or Denoiser(bias_spec) / load_state_dict of a published one
    audio, audio_len = denoiser(*vocoder(mel, mel_len))
"""
from __future__ import annotations

import math
from typing import Optional, Union

import numpy as np
import torch
from torch import Tensor

from . import runtime
from .data.features import twiddles

N_FFT, HOP, BINS = runtime.DENOISE_N_FFT, runtime.DENOISE_HOP, runtime.DENOISE_N_FFT // 2 + 1
MIN_SAMPLES = N_FFT // 2 + 1        # below this the reflect padding is undefined


def hann_window() -> np.ndarray:
    """float64 [1024]: the periodic Hann window."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)


def denoise_tables() -> Tensor:
    """fp32 [5120] for ispk_denoise_f32: W_2048^m as (re, im), then the window; float64, rounded once."""
    return torch.cat([twiddles().flatten(), torch.from_numpy(hann_window().astype(np.float32))]).contiguous()


def frame0_magnitude(x: np.ndarray) -> np.ndarray:
    """float64 [513]: |X_0[k]| of the definition above for a waveform of at least 513 samples."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or x.shape[0] < MIN_SAMPLES:
        raise ValueError(f"frame 0 needs one waveform of at least {MIN_SAMPLES} samples, got shape {x.shape}")
    idx = np.abs(np.arange(N_FFT) - N_FFT // 2)            # r(j - 512): only the reflection at 0 is reached
    return np.abs(np.fft.rfft(x[idx] * hann_window()))


class Denoiser(torch.nn.Module):
    """`Denoiser(bias_spec, strength=0.01)`: bias_spec [513], [513, 1] or [1, 513, 1], non-negative and finite, kept as the
    fp32 buffer `bias_spec` [1, 513, 1] (the key and shape of the published denoisers).  filter_length, hop_length, win_length
    and n_overlap are accepted for compatibility; only 1024 / 256 / 1024 / 4 are built."""

    def __init__(self, bias_spec, strength: float = 0.01, filter_length: int = N_FFT, hop_length: int = HOP,
                 win_length: int = N_FFT, n_overlap: int = N_FFT // HOP):
        super().__init__()
        for name, got, want in (("filter_length", filter_length, N_FFT), ("hop_length", hop_length, HOP),
                                ("win_length", win_length, N_FFT), ("n_overlap", n_overlap, N_FFT // HOP)):
            if got != want:
                raise NotImplementedError(f"{name} {got}: only {name} {want} is built (STFT 1024 / 256 / 1024, 4 overlaps)")
        b = torch.as_tensor(bias_spec).detach()
        if tuple(b.shape) not in ((BINS,), (BINS, 1), (1, BINS, 1)):
            raise ValueError(f"bias_spec: [{BINS}], [{BINS}, 1] or [1, {BINS}, 1], got {tuple(b.shape)}")
        b = b.to("cpu", torch.float32).reshape(1, BINS, 1).clone()
        if not bool(torch.isfinite(b).all()) or bool((b < 0).any()):
            raise ValueError("bias_spec: a magnitude spectrum, every value finite and >= 0")
        self.strength = _check_strength(strength)
        self.register_buffer("bias_spec", b)
        self.register_buffer("tables", denoise_tables(), persistent=False)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """The published denoisers also carry their STFT's conv bases (`stft.*`): those are tables here, not state."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("stft.")}, strict, **kw)

    @classmethod
    def from_vocoder(cls, vocoder, mode: str = "zeros", frames: Optional[int] = None, seed: int = 0,
                     strength: float = 0.01) -> "Denoiser":
        """Runs `vocoder` (Vocoder, HifiGan, BigVGan or IstftNet, on the GPU) once on a [1, n_mels, frames] mel of zeros, or of
        standard-normal values from `seed` (mode "normal"), and keeps |X_0[k]| of frame 0 of that waveform, computed on the
        host in float64 and rounded once.  Construction, outside any forward, as the weight-norm folding is."""
        if mode not in ("zeros", "normal"):
            raise ValueError(f"mode {mode!r}: 'zeros' or 'normal'")
        hop = int(vocoder.hop_length)
        frames = max(88, math.ceil(2 * N_FFT / hop)) if frames is None else int(frames)
        if mode == "zeros":
            mel = torch.zeros((1, vocoder.n_mels, frames), dtype=torch.float32)
        else:
            mel = torch.randn((1, vocoder.n_mels, frames), dtype=torch.float32, generator=torch.Generator().manual_seed(seed))
        dev = next(vocoder.parameters()).device
        with torch.no_grad():
            audio, audio_len = vocoder(mel.to(dev))
        n = int(audio_len[0])
        if n < MIN_SAMPLES:
            raise ValueError(f"{frames} frames of hop {hop} give {n} samples: frame 0 needs at least {MIN_SAMPLES}")
        bias = frame0_magnitude(audio[0, :n].cpu().numpy())
        return cls(torch.from_numpy(bias.astype(np.float32)), strength=strength).to(dev)

    def forward(self, audio: Tensor, audio_len: Optional[Tensor] = None, strength: Union[None, float, Tensor] = None,
                out: Optional[Tensor] = None) -> tuple[Tensor, Optional[Tensor]]:
        """audio fp32 [B, S] on the GPU with int64 lengths [B] -> (denoised fp32 [B, S], audio_len passed through).  strength:
        None (the module's), a float, or an fp32 [B] device tensor with one value per utterance."""
        if not audio.is_cuda or not self.bias_spec.is_cuda:
            raise runtime.IspkError("Denoiser needs GPU tensors and a module on the GPU; there is no CPU fallback")
        s = self.strength if strength is None else strength if isinstance(strength, Tensor) else _check_strength(strength)
        return runtime.denoise(audio, audio_len, self.tables, self.bias_spec.view(BINS), s, out=out), audio_len


def _check_strength(strength) -> float:
    s = float(strength)
    if not s >= 0.0:
        raise ValueError(f"strength {strength}: negative or NaN")
    return s
