"""Loading at another sample rate, batched on the GPU: what `AudioProvider.__call__` (data/providers.py:203-212 of the
reference) does with `torchaudio.transforms.Resample(rate, sample_rate)` and the mean over channels, as ONE launch of
ispk_resample_f32 (csrc/audio.hip).  torchaudio is not a dependency: its "sinc_interp_hann" kernel is restated below from
its documented algorithm, evaluated in float64 and rounded once to fp32 (the reference builds its taps in fp32; that is not
copied).  Channels are averaged BEFORE the filter (equal in exact arithmetic, 1 / C of the work).

`AudioFrontEnd(resampler, features)` chains it with `AcousticFeatures` behind the interface train.GraphedTrainStep(features=)
uses, so a captured training step can start from audio at the file's rate.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .. import runtime

MAX_TABLE_FLOATS = 12288     # ispk_resample_f32 keeps the whole tap table in LDS
MAX_PHASES = 1024
MAX_BLOCK_SPAN = 8184        # ... and 2 width + o input samples of one output block


def sinc_hann_taps(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(k float64 [n, 2 width + o], t float64 of the same shape (unclamped), o, n, width): torchaudio's sinc_interp_hann
    polyphase kernel.  g = gcd, o = orig / g, n = new / g, base = min(o, n) rolloff, width = ceil(lpw o / base);
    t = (-p / n + (j - width) / o) base clamped to +-lpw; k[p, j] = sinc(t) cos^2(pi t / (2 lpw)) base / o."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    lpw = int(lowpass_filter_width)
    base = min(o, n) * float(rolloff)
    width = int(math.ceil(lpw * o / base))
    j = np.arange(2 * width + o, dtype=np.float64)[None, :]
    p = np.arange(n, dtype=np.float64)[:, None]
    t_raw = (-p / n + (j - width) / o) * base
    t = np.clip(t_raw, -lpw, lpw)
    window = np.cos(t * math.pi / lpw / 2.0) ** 2
    tp = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(tp == 0.0, 1.0, np.sin(tp) / np.where(tp == 0.0, 1.0, tp))
    return sinc * window * (base / o), t_raw, o, n, width


def compact_taps(k: np.ndarray, t_raw: np.ndarray, lpw: int):
    """Dense float64 [n, J] -> (fp32 [n, T], int32 first [n]): per phase the run of taps with |t| < lpw (the others are the
    clamp's cos(pi / 2)^2 residue, below 1e-30), zero-filled to the longest run T and kept inside [0, J)."""
    n, J = k.shape
    live = np.abs(t_raw) < lpw
    T = int(live.sum(1).max())
    first = np.minimum(np.argmax(live, axis=1), J - T).astype(np.int64)
    idx = first[:, None] + np.arange(T)[None, :]
    rows = np.arange(n)[:, None]
    taps = np.where(live[rows, idx], k[rows, idx], 0.0)
    assert int((taps != 0).sum()) <= int(live.sum()) and (np.diff(live.astype(np.int8), axis=1) != 0).sum(1).max() <= 2
    return taps.astype(np.float32), first.astype(np.int32)


def resampled_length(length: int, o: int, n: int) -> int:
    """ceil(n length / o): torchaudio's target length."""
    return runtime.resampled_samples(int(length), o, n)


class Resampler:
    """Polyphase windowed-sinc resampling with a fused downmix.

    rs = Resampler(48000, 22050);  audio_out, audio_len_out = rs(audio, audio_len)
      audio      fp32 [B, S] or [B, C, S] on the GPU (unit stride on S); nothing at or past audio_len[b] is read
      audio_len  int64 [B] on the GPU
      audio_out  fp32 [B, ceil(n S / o)]: utterance b's ceil(n audio_len[b] / o) samples, then zeros; audio_len_out int64 [B].
                 A length below 0 or above S gives length 0 and a zero row (lengths are device data).
    Equal rates return mono input untouched and only average the channels of [B, C, S] input.
    The tap table lives in the kernel's LDS: a pair whose table exceeds 12,288 floats (or 1,024 phases, or whose output
    block spans more than 8,184 input samples) raises NotImplementedError.  Every pair among 8, 16, 22.05, 24, 32, 44.1
    and 48 kHz fits (at most 8,320 floats)."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq <= 0 or new_freq <= 0:
            raise ValueError(f"sample rates are positive integers, got {orig_freq!r} -> {new_freq!r}")
        if lowpass_filter_width <= 0 or not 0.0 < rolloff <= 1.0:
            raise ValueError(f"lowpass_filter_width > 0 and 0 < rolloff <= 1, got {lowpass_filter_width!r}, {rolloff!r}")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.lowpass_filter_width, self.rolloff = int(lowpass_filter_width), float(rolloff)
        self.identity = self.orig_freq == self.new_freq
        if self.identity:      # the downmix alone: one tap of 1
            self.o = self.n = 1
            self.width = 0
            self.taps, self.first = torch.ones((1, 1), dtype=torch.float32), torch.zeros((1,), dtype=torch.int32)
        else:
            g = math.gcd(self.orig_freq, self.new_freq)
            self.o, self.n = self.orig_freq // g, self.new_freq // g
            self.width = int(math.ceil(self.lowpass_filter_width * self.o / (min(self.o, self.n) * self.rolloff)))
            if self.n > MAX_PHASES or 2 * self.width + self.o > MAX_BLOCK_SPAN:
                raise NotImplementedError(f"{orig_freq} -> {new_freq} Hz: {self.n} phases over {2 * self.width + self.o} input "
                                          f"samples; at most {MAX_PHASES} phases and {MAX_BLOCK_SPAN} samples are built")
            k, t_raw, _, _, width = sinc_hann_taps(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff)
            assert width == self.width
            taps, first = compact_taps(k, t_raw, self.lowpass_filter_width)
            if taps.size > MAX_TABLE_FLOATS:
                raise NotImplementedError(f"{orig_freq} -> {new_freq} Hz: a tap table of {taps.size} floats; at most "
                                          f"{MAX_TABLE_FLOATS} (the kernel keeps it in LDS) are built")
            self.taps, self.first = torch.from_numpy(taps), torch.from_numpy(first)
        self.T = int(self.taps.shape[1])
        self._on: dict = {}

    def out_samples(self, S: int) -> int:
        return resampled_length(S, self.o, self.n)

    def device_tables(self, device) -> tuple[Tensor, Tensor]:
        """(taps, first) on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = (self.taps.to(device), self.first.to(device))
        return t

    def empty_outputs(self, B: int, S: int, device) -> tuple[Tensor, Tensor]:
        return (torch.empty((B, self.out_samples(S)), dtype=torch.float32, device=device),
                torch.empty((B,), dtype=torch.int64, device=device))

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[tuple] = None) -> tuple[Tensor, Tensor]:
        if audio.ndim not in (2, 3) or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] or [B, C, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} "
                             f"strides {tuple(audio.stride())}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not audio.is_cuda or not audio_len.is_cuda:
            raise runtime.IspkError("Resampler needs GPU tensors; there is no CPU fallback")
        if self.identity and audio.ndim == 2 and out is None:
            return audio, audio_len
        taps, first = self.device_tables(audio.device)
        o_audio, o_len = out if out is not None else (None, None)
        return runtime.resample(audio, audio_len, taps, first, self.o, self.n, self.width, o_audio, o_len)


class AudioFrontEnd:
    """Resampler, then AcousticFeatures, as one callable with the interface train.GraphedTrainStep(features=) uses: two
    launches, no ATen compute op, no host read.  Mono [B, S] at the resampler's input rate; S is the INPUT width.

    The returned dict is the extractor's (mel, mel_len, pitch, energy) plus "audio_resampled" / "audio_resampled_len".

    With `conditioner` (data.AudioConditioner at the extractor's rate) the order is resample, condition, extract: the
    extractor sees the trimmed, loudness-normalised audio, which the dict also returns as "audio_conditioned" /
    "audio_conditioned_len" (four more launches).  Without one nothing changes."""

    def __init__(self, resampler: Resampler, features, conditioner=None):
        if resampler.new_freq != features.sample_rate:
            raise ValueError(f"the resampler delivers {resampler.new_freq} Hz, the extractor expects {features.sample_rate} Hz")
        if conditioner is not None and conditioner.sample_rate != features.sample_rate:
            raise ValueError(f"the conditioner meters at {conditioner.sample_rate} Hz, the extractor expects {features.sample_rate} Hz")
        self.resampler, self.features, self.conditioner = resampler, features, conditioner

    @property
    def pitch(self) -> bool:
        return self.features.pitch

    @property
    def energy(self) -> bool:
        return self.features.energy

    def device_tables(self, device):
        t = self.resampler.device_tables(device), self.features.device_tables(device)
        return t if self.conditioner is None else t + (self.conditioner.device_tables(device),)

    def empty_outputs(self, B: int, S: int, device) -> dict:
        a, ln = self.resampler.empty_outputs(B, S, device)
        out = dict(self.features.empty_outputs(B, a.shape[1], device), audio_resampled=a, audio_resampled_len=ln)
        if self.conditioner is not None:
            c = self.conditioner.empty_outputs(B, a.shape[1], device)
            out.update(audio_conditioned=c.pop("audio"), audio_conditioned_len=c.pop("audio_len"), **c)
        return out

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        if audio.ndim != 2:
            raise ValueError(f"AudioFrontEnd takes mono fp32 [B, S]; use Resampler for [B, C, S], got {tuple(audio.shape)}")
        if out is None:
            out = self.empty_outputs(audio.shape[0], audio.shape[1], audio.device)
        a, ln = self.resampler(audio, audio_len, out=(out["audio_resampled"], out["audio_resampled_len"]))
        if self.conditioner is not None:
            c = dict(out, audio=out["audio_conditioned"], audio_len=out["audio_conditioned_len"])
            self.conditioner(a, ln, out=c)
            a, ln = c["audio"], c["audio_len"]
        self.features(a, ln, out=out)
        return out
