"""Griffin-Lim mel inversion: waveforms from mel spectrograms without a vocoder checkpoint, with the vocoders' call surface.

The framing is data.AcousticFeatures' own STFT (csrc/features.hip): N = 1024, hop 256, K = 513 bins, w the periodic Hann
window, 384 zeros on both sides, no centring - so the result is the waveform whose extractor mel the iteration drives toward
the input.  An utterance of T = mel_len[b] frames has n = 256 T samples; with xp[p] = x[p - 384] inside [0, n) and 0 elsewhere:

    mel -> magnitude   M_f[k] = max(sum_m P[k][m] exp(mel[m][f]), 0), P the Moore-Penrose pseudo-inverse of the extractor's
                       filterbank melscale_fbanks(...)^T, made on the host in float64 at construction and rounded once (the
                       least-squares solution of torchaudio's InverseMelScale, then its relu)
    analysis           X_f[k] = sum_j xp[256 f + j] w[j] exp(-2 pi i j k / 1024),  f < T, k <= 512
    projection         Y_f[k] = M_f[k] X_f[k] / |X_f[k]|, M_f[k] where |X_f[k]| = 0
    synthesis          y_f = irfft(Y_f);  out[s] = sum_f w[j] y_f[j] / sum_f w[j]^2, j = s + 384 - 256 f, over the utterance's
                       own frames in ascending order; 0 from n on
    initial waveform   synthesis alone of Y_f[k] = M_f[k] exp(2 pi i u), u = (h >> 8) 2^-24, h = drop_hash(mix_seed(seed),
                       513 f + k) of csrc/dropout.h: a function of (seed, f, k) only

One call is one launch of ispk_mel_to_linear_f32, one of ispk_griffinlim_step_f32 in mode init and n_iter in mode step
(csrc/griffinlim.hip; analysis, projection and synthesis of a 4,096-sample tile in one launch, nothing in HBM between them):
no ATen compute, no host read, one stream, capturable with out=, and an utterance's samples do not depend on its batch.

GriffinLim is the plain iteration (momentum 0).  FastGriffinLim is the fast one (torchaudio's and librosa's default, momentum
0.99): the textbook form keeps tprev = STFT(x_{n-1}) and takes the phase of STFT(x_n) - a tprev, a = momentum / (1 + momentum).
The STFT is linear, so that is STFT(x_n - a x_{n-1}): the fast iteration is the same single-launch projection applied to
x_n - a x_{n-1} (ispk_griffinlim_fast_step_f32: one more waveform read per sample, no spectrum in memory, one launch per
iteration; in float64 the two forms agree to 3e-12 of the peak after 32 iterations).  With x_{-1} = 0 the first iteration is
the plain step.  spectral_convergence() is || |STFT(x)| - M ||_F / || M ||_F per utterance on the device
(ispk_griffinlim_error_f32, two launches, no atomics), capturable like the rest.

    gl = GriffinLim.from_features(feats).to("cuda")           # or GriffinLim(sample_rate=22050, n_mels=80, ...)
    audio, audio_len = gl(mel, mel_len)
    fast = FastGriffinLim.from_features(feats, momentum=0.99).to("cuda")
    audio, audio_len = fast(mel, mel_len)
    sc = fast.spectral_convergence(audio, fast.magnitude(mel, mel_len), mel_len)      # fp32 [B]
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import runtime
from .data.features import melscale_fbanks
from .denoiser import denoise_tables

N_FFT, HOP, PAD, BINS = runtime.GRIFFINLIM_N_FFT, runtime.GRIFFINLIM_HOP, runtime.GRIFFINLIM_PAD, runtime.GRIFFINLIM_N_FFT // 2 + 1


def filterbank_pinv(fb) -> np.ndarray:
    """float64 [513, n_mels]: the Moore-Penrose pseudo-inverse P of fb^T, fb [513, n_mels] the extractor's filterbank
    (mel = fb^T magnitude), so that P mel is the least-squares magnitude."""
    fb = np.asarray(fb, dtype=np.float64)
    if fb.ndim != 2 or fb.shape[0] != BINS:
        raise ValueError(f"filterbank: [{BINS}, n_mels], got {fb.shape}")
    return np.linalg.pinv(fb.T)


class GriffinLim(torch.nn.Module):
    """`GriffinLim(sample_rate=22050, n_mels=80, f_min=0.0, f_max=8000.0, n_iter=32, seed=0)`: the filterbank is
    AcousticFeatures' for the same arguments.  n_fft, hop_length, win_length, window, momentum, mel_scale and norm are accepted
    for compatibility; only 1024 / 256 / 1024, "hann", 0, "slaney" and "slaney" are built (a momentum: FastGriffinLim)."""

    def __init__(self, sample_rate: int = 22050, n_mels: int = 80, f_min: float = 0.0, f_max: Optional[float] = 8000.0,
                 n_iter: int = 32, seed: int = 0, n_fft: int = N_FFT, hop_length: int = HOP, win_length: int = N_FFT,
                 window: str = "hann", momentum: float = 0.0, mel_scale: str = "slaney", norm: Optional[str] = "slaney",
                 _fb: Optional[Tensor] = None):
        super().__init__()
        for name, got, want in (("n_fft", n_fft, N_FFT), ("hop_length", hop_length, HOP), ("win_length", win_length, N_FFT),
                                ("window", window, "hann"), ("mel_scale", mel_scale, "slaney"), ("norm", norm, "slaney")):
            if got != want:
                raise NotImplementedError(f"{name} {got!r}: only {name} {want!r} is built (the feature extractor's STFT, "
                                          f"1024 / 256 / 1024 periodic Hann, and its slaney filterbank)")
        if float(momentum) != 0.0:
            raise NotImplementedError(f"momentum {momentum}: GriffinLim is the plain iteration (momentum 0); FastGriffinLim "
                                      f"is the fast one (by linearity of the STFT, the same projection applied to x_n - a "
                                      f"x_(n-1), a = momentum / (1 + momentum))")
        self.sample_rate, self.n_mels, self.hop_length = int(sample_rate), int(n_mels), HOP
        if not 1 <= self.n_mels <= 128:
            raise NotImplementedError(f"n_mels={n_mels}: 1 .. 128 mel channels are built")
        self.n_iter, self.seed = _check_iter(n_iter), _check_seed(seed)
        fb = _fb if _fb is not None else melscale_fbanks(BINS, float(f_min), float(f_max if f_max is not None else
                                                                                   self.sample_rate // 2),
                                                         self.n_mels, self.sample_rate, "slaney", "slaney")
        if tuple(fb.shape) != (BINS, self.n_mels):
            raise ValueError(f"filterbank: [{BINS}, {self.n_mels}], got {tuple(fb.shape)}")
        pinv = filterbank_pinv(fb.double().numpy())
        self.register_buffer("pinv_t", torch.from_numpy(np.ascontiguousarray(pinv.T).astype(np.float32)), persistent=False)
        self.register_buffer("tables", denoise_tables(), persistent=False)

    @classmethod
    def from_features(cls, features, n_iter: int = 32, seed: int = 0) -> "GriffinLim":
        """The inversion of a data.AcousticFeatures: its sample rate, channel count and filterbank."""
        return cls(sample_rate=features.sample_rate, n_mels=features.n_mels, n_iter=n_iter, seed=seed, _fb=features.fb)

    # ---- forward
    def empty_outputs(self, B: int, T: int, device) -> tuple[Tensor, Tensor]:
        return (torch.empty((B, T * HOP), dtype=torch.float32, device=device),
                torch.empty((B,), dtype=torch.int64, device=device))

    def _on_gpu(self, *tensors) -> None:
        if not self.pinv_t.is_cuda or any(t is not None and not t.is_cuda for t in tensors):
            raise runtime.IspkError("GriffinLim needs GPU tensors and a module on the GPU; there is no CPU fallback")

    def magnitude(self, mel: Tensor, mel_len: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
        """mel fp32 / fp16 [B, n_mels, T] -> the magnitude fp32 [B, T, 513]; frames at or past mel_len are left unwritten."""
        self._on_gpu(mel, mel_len, out)
        if mel.ndim != 3 or mel.dtype not in (torch.float32, torch.float16) or mel.shape[1] != self.n_mels:
            raise ValueError(f"mel: fp32 / fp16 [B, {self.n_mels}, T], got {mel.dtype} {tuple(mel.shape)}")
        return runtime.mel_to_linear(mel, mel_len, self.pinv_t, out=out)

    def _iteration(self, mag, mel_len, init, n_iter, seed, out):
        """from_magnitude's checked arguments -> (n_iter, seed, audio, audio_len); without frames audio_len is zeroed here and
        nothing remains to launch."""
        self._on_gpu(mag, mel_len, init, *(out or ()))
        n_iter = self.n_iter if n_iter is None else _check_iter(n_iter)
        seed = self.seed if seed is None else _check_seed(seed)
        if mag.ndim != 3:
            raise ValueError(f"magnitude: fp32 [B, T, {BINS}], got {tuple(mag.shape)}")
        B, T = mag.shape[:2]
        audio, audio_len = out if out is not None else self.empty_outputs(B, T, mag.device)
        if init is not None and n_iter == 0:
            raise ValueError("init with n_iter = 0: there is nothing to iterate")
        if B > 0 and T == 0:
            runtime.zero_(audio_len)
        return n_iter, seed, audio, audio_len

    def from_magnitude(self, mag: Tensor, mel_len: Optional[Tensor] = None, init: Optional[Tensor] = None,
                       n_iter: Optional[int] = None, seed: Optional[int] = None,
                       out: Optional[tuple[Tensor, Tensor]] = None) -> tuple[Tensor, Tensor]:
        """The iteration on a given magnitude fp32 [B, T, 513] -> (audio fp32 [B, 256 T], audio_len = 256 mel_len).  `init`: a
        waveform batch fp32 [B, 256 T] to start from in place of the hashed phase (n_iter >= 1; it is not modified).  The
        iterations ping-pong between `out` and one scratch batch so that the last lands in `out`, whatever the parity of
        n_iter; n_iter = 0 returns the initial waveform."""
        n_iter, seed, audio, audio_len = self._iteration(mag, mel_len, init, n_iter, seed, out)
        B, T = mag.shape[:2]
        if B == 0 or T == 0:
            return audio, audio_len
        scratch = torch.empty((B, T * HOP), dtype=torch.float32, device=mag.device) if n_iter >= 1 else None
        # iterate i (0 = the initial waveform) lives in `audio` when n_iter - i is even
        cur = init
        if init is None:
            cur = audio if n_iter % 2 == 0 else scratch
            runtime.griffinlim_step(None, mag, mel_len, self.tables, cur, audio_len=audio_len if n_iter == 0 else None,
                                    mode=runtime.GRIFFINLIM_INIT, seed=seed)
        for i in range(1, n_iter + 1):
            nxt = audio if (n_iter - i) % 2 == 0 else scratch
            runtime.griffinlim_step(cur, mag, mel_len, self.tables, nxt, audio_len=audio_len if i == n_iter else None)
            cur = nxt
        return audio, audio_len

    def spectral_convergence(self, audio: Tensor, mag: Tensor, mel_len: Optional[Tensor] = None,
                             out: Optional[Tensor] = None) -> Tensor:
        """|| |STFT(audio)| - mag ||_F / || mag ||_F per utterance over its mel_len frames, in the iteration's own framing:
        audio fp32 [B, 256 T], mag fp32 [B, T, 513] -> fp32 [B].  0 for an utterance without frames; with an all-zero
        magnitude, 0 under silence and +inf otherwise."""
        self._on_gpu(audio, mag, mel_len, out)
        return runtime.griffinlim_error(audio, mag, mel_len, self.tables, out=out)

    def forward(self, mel: Tensor, mel_len: Optional[Tensor] = None,
                out: Optional[tuple[Tensor, Tensor]] = None) -> tuple[Tensor, Tensor]:
        """mel fp32 / fp16 [B, n_mels, T] on the GPU -> (audio fp32 [B, 256 T], audio_len int64 [B] = 256 mel_len)."""
        mag = self.magnitude(mel, mel_len)
        return self.from_magnitude(mag, mel_len, out=out)

    @torch.no_grad()
    def infer(self, mel: Tensor) -> Tensor:
        """`gl.infer(mel)`: every utterance has all T frames; audio fp32 [B, 256 T]."""
        return self.forward(mel)[0]


class FastGriffinLim(GriffinLim):
    """`FastGriffinLim(..., momentum=0.99)`: GriffinLim's arguments and call surface, the fast iteration with 0 <= momentum < 1
    (0: the plain iteration, bit for bit)."""

    def __init__(self, *args, momentum: float = 0.99, **kwargs):
        super().__init__(*args, **kwargs)
        self.momentum = _check_momentum(momentum)

    @classmethod
    def from_features(cls, features, n_iter: int = 32, seed: int = 0, momentum: float = 0.99) -> "FastGriffinLim":
        return cls(sample_rate=features.sample_rate, n_mels=features.n_mels, n_iter=n_iter, seed=seed, momentum=momentum,
                   _fb=features.fb)

    def from_magnitude(self, mag: Tensor, mel_len: Optional[Tensor] = None, init: Optional[Tensor] = None,
                       n_iter: Optional[int] = None, seed: Optional[int] = None,
                       out: Optional[tuple[Tensor, Tensor]] = None, momentum: Optional[float] = None) -> tuple[Tensor, Tensor]:
        """GriffinLim.from_magnitude with the fast iteration.  x_0 is the hashed start or `init` (not modified) and x_{-1} = 0:
        iteration 1 is the plain step, iteration i >= 2 the fast step on (x_{i-1}, x_{i-2}).  The iterates rotate over `out`
        and two scratch batches so that the last lands in `out` for every n_iter."""
        momentum = self.momentum if momentum is None else _check_momentum(momentum)
        if momentum == 0.0:
            return super().from_magnitude(mag, mel_len, init=init, n_iter=n_iter, seed=seed, out=out)
        n_iter, seed, audio, audio_len = self._iteration(mag, mel_len, init, n_iter, seed, out)
        B, T = mag.shape[:2]
        if B == 0 or T == 0:
            return audio, audio_len
        alpha = float(np.float32(momentum / (1.0 + momentum)))         # float64, rounded once
        ring = [audio, None, None]                                        # iterate i lives in ring[(n_iter - i) % 3]

        def slot(i):
            j = (n_iter - i) % 3
            if ring[j] is None:
                ring[j] = torch.empty((B, T * HOP), dtype=torch.float32, device=mag.device)
            return ring[j]

        cur, prev = init, None
        if init is None:
            cur = slot(0)
            runtime.griffinlim_step(None, mag, mel_len, self.tables, cur, audio_len=audio_len if n_iter == 0 else None,
                                    mode=runtime.GRIFFINLIM_INIT, seed=seed)
        for i in range(1, n_iter + 1):
            nxt, last = slot(i), audio_len if i == n_iter else None
            if i == 1:
                runtime.griffinlim_step(cur, mag, mel_len, self.tables, nxt, audio_len=last)
            else:
                runtime.griffinlim_fast_step(cur, prev, alpha, mag, mel_len, self.tables, nxt, audio_len=last)
            cur, prev = nxt, cur
        return audio, audio_len


def _check_momentum(momentum) -> float:
    m = float(momentum)
    if not 0.0 <= m < 1.0:
        raise ValueError(f"momentum {momentum}: 0 <= momentum < 1")
    return m


def _check_iter(n_iter) -> int:
    n = int(n_iter)
    if n != n_iter or n < 0:
        raise ValueError(f"n_iter {n_iter}: a non-negative integer")
    return n


def _check_seed(seed) -> int:
    s = int(seed)
    if s != seed or not 0 <= s < 2 ** 64:
        raise ValueError(f"seed {seed}: an unsigned 64-bit integer")
    return s
