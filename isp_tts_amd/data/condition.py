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


def true_peak_taps() -> np.ndarray:
    """float64 [4, 12]: the 4x interpolator of the true-peak detector.  Row p, column k + 5 holds h[p][k] = sinc(t) cos^2(pi t /
    12) for |t| < 6, else 0, with t = k - p / 4, k = -5 .. 6: a windowed sinc of six samples to each side.  Row 0 is exactly
    the identity; rows 1 and 3 mirror each other.  The kernel takes the table as fp32."""
    t = np.arange(-5, 7, dtype=np.float64)[None, :] - np.arange(4, dtype=np.float64)[:, None] / 4.0
    h = np.where(np.abs(t) < 6.0, np.sinc(t) * np.cos(np.pi * t / 12.0) ** 2, 0.0)
    h[0] = 0.0
    h[0, 5] = 1.0            # sinc of a non-zero integer is zero up to an ulp of pi: made exact
    return h


class Limiter:
    """A look-ahead limiter with a true-peak (4x oversampled) detector, one launch of ispk_limit_f32 (csrc/limiter.hip) with
    no ATen compute op and no host read: the gain is pulled down, smoothly and ahead of time, only over the stretches whose
    inter-sample peak would exceed the ceiling; everything else keeps its bits.

    lim = Limiter(sample_rate, ceiling_db=-1.0, lookahead_ms=1.5)
    r = lim(audio, audio_len, gain=None, bounds=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride) and int64 [B] on the GPU; a length outside [0, S] counts as 0
      gain, bounds       fp32 [B] and int64 [B, 2], an AudioConditioner's: the item is audio[start, end) times gain
      r["audio"]         fp32 [B, S]: clamp(gain x s, -ceiling, ceiling), zeros behind the item;  r["audio_len"] int64 [B]
      r["true_peak"]     fp32 [B]: the largest 4x interpolated magnitude of gain x, BEFORE limiting (0 for an empty item)
      r["reduction"]     fp32 [B]: the smallest gain s applied (1.0: untouched)
    With e[i] the largest magnitude among sample i and its three interpolated successors, r = ceiling / e where e exceeds the
    ceiling (else 1), m the minimum of r over +-lookahead samples and s = 1 - sum w (1 - m) over another +-lookahead with a
    raised-cosine w that sums to one (include/ispk.h has it in full): s <= r at every sample, so no output SAMPLE exceeds the
    ceiling, and s is exactly 1 further than 2 lookahead from anything limited.  `.lookahead` is the rounded sample count
    (1 .. 256), `.ceiling` the linear ceiling as the kernel takes it (rounded to fp32)."""

    def __init__(self, sample_rate: int, ceiling_db: float = -1.0, lookahead_ms: float = 1.5):
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
        if not math.isfinite(ceiling_db):
            raise ValueError(f"ceiling_db is finite, got {ceiling_db!r}")
        if not (lookahead_ms > 0 and math.isfinite(lookahead_ms)):
            raise ValueError(f"lookahead_ms > 0, got {lookahead_ms!r}")
        self.sample_rate, self.ceiling_db, self.lookahead_ms = int(sample_rate), float(ceiling_db), float(lookahead_ms)
        self.ceiling = float(np.float32(10.0 ** (self.ceiling_db / 20.0)))
        if not (self.ceiling > 0 and math.isfinite(self.ceiling)):
            raise ValueError(f"ceiling_db {ceiling_db!r} is not a positive finite fp32 ceiling")
        self.lookahead = int(round(self.lookahead_ms * 1e-3 * self.sample_rate))
        if not 1 <= self.lookahead <= runtime.LIMIT_MAX_LOOKAHEAD:
            raise ValueError(f"lookahead_ms {lookahead_ms!r} is {self.lookahead} samples at {self.sample_rate} Hz: 1 .. "
                             f"{runtime.LIMIT_MAX_LOOKAHEAD}")
        self.taps = torch.from_numpy(true_peak_taps().astype(np.float32))
        self._on: dict = {}

    def device_tables(self, device) -> Tensor:
        """The interpolator taps (fp32 [4, 12]) on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.taps.to(device)
        return t

    def empty_outputs(self, B: int, S: int, device) -> dict:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)      # noqa: E731
        return dict(audio=e((B, S), torch.float32), audio_len=e((B,), torch.int64), true_peak=e((B,), torch.float32),
                    reduction=e((B,), torch.float32))

    def _checked(self, audio: Tensor, audio_len: Tensor, gain: Optional[Tensor], bounds: Optional[Tensor]) -> None:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        for t in (audio, audio_len, gain, bounds):
            if t is not None and not t.is_cuda:
                raise runtime.IspkError("Limiter needs GPU tensors; there is no CPU fallback")

    def __call__(self, audio: Tensor, audio_len: Tensor, gain: Optional[Tensor] = None, bounds: Optional[Tensor] = None,
                 out: Optional[dict] = None) -> dict:
        self._checked(audio, audio_len, gain, bounds)
        if out is None:
            out = self.empty_outputs(audio.shape[0], audio.shape[1], audio.device)
        runtime.limit(audio, audio_len, self.device_tables(audio.device), self.ceiling, self.lookahead, gain, bounds, out["audio"],
                      out["audio_len"], out["true_peak"], out["reduction"])
        return out

    def true_peak(self, audio: Tensor, audio_len: Tensor, gain: Optional[Tensor] = None) -> Tensor:
        """fp32 [B]: the true peak of gain * audio - the same launch without an output; no audio is written."""
        self._checked(audio, audio_len, gain, None)
        return runtime.limit(audio, audio_len, self.device_tables(audio.device), self.ceiling, self.lookahead, gain,
                             measure_only=True)[2]


class AudioConditioner:
    """Trim, measure and normalise a padded mono batch in four launches (three of ispk_audio_measure_f64, one of
    ispk_audio_apply_f32), with no ATen compute op and no host read.

    cond = AudioConditioner(sample_rate, target_lufs=-23.0, peak_limit=10 ** (-1 / 20), top_db=60.0, pad_frames=0, ref="max",
                            limiter=None)
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
    calls and graph replays are bit-identical.  8 kHz <= sample_rate <= 768 kHz, a multiple of 10 (the 100 ms step).

    With `limiter=Limiter(...)` the loudness gain is not capped by the sample peak (peak_limit is not used): r["gain"] is
    10^((target_lufs - loudness) / 20) itself, and one ispk_limit_f32 launch with the bounds and that gain takes the place of
    ispk_audio_apply_f32 - still four launches.  r["audio"] is then the limited audio, and r gains r["true_peak"] (fp32 [B], of
    the gained item before limiting) and r["reduction"] (fp32 [B], the smallest limiter gain; 1.0: untouched).  r["loudness"]
    stays the measured INPUT loudness; limiting lowers the loudness that is achieved slightly below the target wherever it
    acts, and nothing iterates on that.  limiter=None is the conditioner as it was, bit for bit."""

    def __init__(self, sample_rate: int, target_lufs: Optional[float] = -23.0, peak_limit: float = 10 ** (-1 / 20),
                 top_db: Optional[float] = 60.0, pad_frames: int = 0, ref: Union[str, float] = "max",
                 limiter: Optional[Limiter] = None):
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
        if limiter is not None and not isinstance(limiter, Limiter):
            raise ValueError(f"limiter is a Limiter or None, got {type(limiter).__name__}")
        if limiter is not None and limiter.sample_rate != self.sample_rate:
            raise ValueError(f"limiter: built for {limiter.sample_rate} Hz, the conditioner for {self.sample_rate} Hz")
        self.limiter = limiter
        self.table = torch.from_numpy(meter_table(self.sample_rate))
        self._on: dict = {}

    def device_tables(self, device) -> Tensor:
        """The coefficient / matrix-power table on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.table.to(device)
        if self.limiter is not None:
            self.limiter.device_tables(device)
        return t

    def empty_outputs(self, B: int, S: int, device) -> dict:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        out = dict(audio=e((B, S), torch.float32), audio_len=e((B,), torch.int64), bounds=e((B, 2), torch.int64),
                   loudness=e((B,), torch.float64), peak=e((B,), torch.float32), gain=e((B,), torch.float32))
        if self.limiter is not None:
            out.update(true_peak=e((B,), torch.float32), reduction=e((B,), torch.float32))
        return out

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
                              self.peak_limit if self.limiter is None else math.inf, out["bounds"], out["loudness"], out["peak"],
                              out["gain"])
        if self.limiter is None:
            runtime.audio_apply(audio, out["bounds"], out["gain"], out["audio"], out["audio_len"])
        else:      # the gain uncapped (no peak limit binds), then only the stretches over the ceiling pulled down
            lim = self.limiter
            runtime.limit(audio, audio_len, lim.device_tables(audio.device), lim.ceiling, lim.lookahead, out["gain"], out["bounds"],
                          out["audio"], out["audio_len"], out["true_peak"], out["reduction"])
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
