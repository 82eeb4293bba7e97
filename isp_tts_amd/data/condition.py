"""Audio conditioning, batched on the GPU, the same at both ends of the pipeline: silence trimming, loudness normalisation to
ITU-R BS.1770-4 and conversion to 16-bit PCM (csrc/condition.hip).  The reference has no counterpart: it takes recordings as
they come and returns the vocoder's fp32.

    cond = AudioConditioner(22050);  r = cond(audio, audio_len)          # r["audio"], r["audio_len"], r["loudness"], ...
    pcm = to_pcm16(r["audio"], r["audio_len"])

`AudioFrontEnd(resampler, features, conditioner=cond)` (data.resample) puts it between the resampler and the extractor; behind
the vocoder it is `to_pcm16(*cond(vocoder(mel, mel_len)...))` - see the README.
"""
from __future__ import annotations

import math
from typing import Optional, Union

import numpy as np
import torch
from torch import Tensor

from .. import runtime

SHELF_F0, SHELF_GAIN_DB, SHELF_Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
SHELF_VB_EXPONENT = 0.4996667741545416
HIGHPASS_F0, HIGHPASS_Q = 38.13547087602444, 0.5003270373238773
CHUNK = 32                   # samples per lane of the scan; the table holds A^(CHUNK 2^k), k = 0 .. 8
POWERS = 9


def k_weighting(sample_rate: int):
    """((b, a), (b, a)) float64 [3] each: the K-weighting high shelf and high-pass of BS.1770 at `sample_rate`, from the analogue
    prototypes whose bilinear transform at 48 kHz is the standard's table.  K = tan(pi f0 / fs), a0 = 1 + K / Q + K^2;
    shelf b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0 with Vh = 10^(G / 20), Vb = Vh^0.49966677;
    high-pass b = [1, -2, 1]; both a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]."""
    if int(sample_rate) != sample_rate or sample_rate <= 0:
        raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
    fs = float(sample_rate)
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXPONENT
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = (np.array([(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0]))
    K = math.tan(math.pi * HIGHPASS_F0 / fs)
    a0 = 1.0 + K / HIGHPASS_Q + K * K
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HIGHPASS_Q + K * K) / a0]))
    return shelf, highpass


def meter_table(sample_rate: int) -> np.ndarray:
    """float64 [152] for ispk_audio_measure_f64: b0, b1, b2, a1, a2 of the shelf, a1, a2 of the high-pass, one unused, then
    A^(32 2^k), k = 0 .. 8, row-major: A is the transition of the cascade's four transposed-direct-form-II states
    (s' = A s + B x), read off the kernel's update with x = 0."""
    (b, a), (_, d) = k_weighting(sample_rate)
    A = np.array([[-a[1], 1.0, 0.0, 0.0],
                  [-a[2], 0.0, 0.0, 0.0],
                  [-2.0 - d[1], 0.0, -d[1], 1.0],
                  [1.0 - d[2], 0.0, -d[2], 0.0]], dtype=np.float64)
    P = np.linalg.matrix_power(A, CHUNK)
    out = [np.array([b[0], b[1], b[2], a[1], a[2], d[1], d[2], 0.0])]
    for _ in range(POWERS):
        out.append(P.reshape(-1))
        P = P @ P
    t = np.concatenate(out)
    assert t.shape == (runtime.CONDITION_TABLE_DOUBLES,)
    return t


class AudioConditioner:
    """Trim, measure and normalise a padded mono batch in four launches (three of ispk_audio_measure_f64, one of
    ispk_audio_apply_f32), with no ATen compute op and no host read.

    cond = AudioConditioner(sample_rate, target_lufs=-23.0, peak_limit=10 ** (-1 / 20), top_db=60.0, pad_frames=0, ref="max")
    r = cond(audio, audio_len)
      audio      fp32 [B, S] on the GPU (unit stride on S, any row stride); nothing at or past audio_len[b] is read
      audio_len  int64 [B] on the GPU; a length below 0 or above S counts as 0
      r["bounds"]     int64 [B, 2]: (start, end) of what is kept.  Frames of 1024 samples every 256; a frame is active when its
                      mean square exceeds ref * 10^(-top_db / 10), ref the utterance's largest frame ("max") or a constant;
                      start / end are the first active frame's first and the last one's last sample, widened by pad_frames
                      frames.  No active frame gives (0, 0).  top_db=None keeps (0, audio_len).
      r["loudness"]   float64 [B]: BS.1770-4 gated loudness (LKFS) of audio[start, end), -inf when no 400 ms block passes.
      r["peak"]       fp32 [B]: max |x| over [start, end).
      r["gain"]       fp32 [B]: 10^((target_lufs - loudness) / 20), at most peak_limit / peak; 1 for loudness -inf and with
                      target_lufs=None (the shift alone).
      r["audio"]      fp32 [B, S]: gain * audio[start + i] for i < end - start, then zeros; r["audio_len"] int64 [B] = end - start.
    Filter state, block sums and gates are float64; an item's results do not depend on the batch it is in, and repeated
    calls and graph replays are bit-identical.  8 kHz <= sample_rate <= 768 kHz, a multiple of 10 (the 100 ms step)."""

    def __init__(self, sample_rate: int, target_lufs: Optional[float] = -23.0, peak_limit: float = 10 ** (-1 / 20),
                 top_db: Optional[float] = 60.0, pad_frames: int = 0, ref: Union[str, float] = "max"):
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
        if sample_rate % 10:
            raise ValueError(f"{sample_rate} Hz: the 100 ms step of the loudness meter is not a whole number of samples")
        if not runtime.CONDITION_RATES[0] <= sample_rate <= runtime.CONDITION_RATES[1]:
            raise NotImplementedError(f"{sample_rate} Hz: the meter is built for {runtime.CONDITION_RATES[0]} .. "
                                      f"{runtime.CONDITION_RATES[1]} Hz")
        if target_lufs is not None and not math.isfinite(target_lufs):
            raise ValueError(f"target_lufs is finite or None, got {target_lufs!r}")
        if not (peak_limit > 0 and math.isfinite(peak_limit)):
            raise ValueError(f"peak_limit > 0, got {peak_limit!r}")
        if top_db is not None and not (top_db > 0 and math.isfinite(top_db)):
            raise ValueError(f"top_db > 0 or None, got {top_db!r}")
        if int(pad_frames) != pad_frames or not 0 <= pad_frames <= 65536:
            raise ValueError(f"pad_frames is an integer in [0, 65536], got {pad_frames!r}")
        if not (ref == "max" or (not isinstance(ref, str) and ref > 0 and math.isfinite(ref))):
            raise ValueError(f'ref is "max" or a positive number, got {ref!r}')
        self.sample_rate = int(sample_rate)
        self.target_lufs = None if target_lufs is None else float(target_lufs)
        self.peak_limit, self.top_db, self.pad_frames = float(peak_limit), None if top_db is None else float(top_db), int(pad_frames)
        self.ref = ref if ref == "max" else float(ref)
        if self.top_db is None:
            self.trim_mode, self.trim_threshold = 0, 0.0
        elif self.ref == "max":
            self.trim_mode, self.trim_threshold = 1, 10.0 ** (-self.top_db / 10.0)
        else:
            self.trim_mode, self.trim_threshold = 2, self.ref * 10.0 ** (-self.top_db / 10.0)
        self.table = torch.from_numpy(meter_table(self.sample_rate))
        self._on: dict = {}

    def device_tables(self, device) -> Tensor:
        """The coefficient / matrix-power table on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.table.to(device)
        return t

    def empty_outputs(self, B: int, S: int, device) -> dict:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        return dict(audio=e((B, S), torch.float32), audio_len=e((B,), torch.int64), bounds=e((B, 2), torch.int64),
                    loudness=e((B,), torch.float64), peak=e((B,), torch.float32), gain=e((B,), torch.float32))

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not audio.is_cuda or not audio_len.is_cuda:
            raise runtime.IspkError("AudioConditioner needs GPU tensors; there is no CPU fallback")
        if out is None:
            out = self.empty_outputs(audio.shape[0], audio.shape[1], audio.device)
        table = self.device_tables(audio.device)
        runtime.audio_measure(audio, audio_len, table, self.sample_rate, self.trim_mode, self.trim_threshold, self.pad_frames,
                              int(self.target_lufs is not None), self.target_lufs if self.target_lufs is not None else 0.0,
                              self.peak_limit, out["bounds"], out["loudness"], out["peak"], out["gain"])
        runtime.audio_apply(audio, out["bounds"], out["gain"], out["audio"], out["audio_len"])
        return out


def to_pcm16(audio: Tensor, audio_len: Tensor, dither: bool = False, seed: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """fp32 [B, S] -> int16 [B, S] in one launch of ispk_pcm16: q = clamp(rint(32768 x + d), -32768, 32767), rounding half to
    even; samples at or past audio_len[b] give 0.  d = 0, or with dither=True the TPDF of +-1 LSB d = u1 - u2, u1 and u2 the
    mix32 hashes (csrc/dropout.h) of (seed, b, 2 i) and (seed, b, 2 i + 1) scaled by 2^-32.

    The dither is a pure function of (seed, b, i): two calls with one seed are equal, and a captured graph REPEATS its dither
    on every replay (the seed is a launch argument, frozen at capture).  Capture one graph per seed, or call eagerly, where
    successive utterances must not share a dither sequence."""
    if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
        raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    if int(seed) != seed or seed < 0:
        raise ValueError(f"seed is a non-negative integer, got {seed!r}")
    if not audio.is_cuda or not audio_len.is_cuda:
        raise runtime.IspkError("to_pcm16 needs GPU tensors; there is no CPU fallback")
    return runtime.pcm16(audio, audio_len, dither, seed, out)
