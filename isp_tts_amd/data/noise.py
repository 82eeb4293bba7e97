"""NoiseReducer: stationary noise reduction (room tone, fan, preamp hiss) on the GPU (csrc/noise.hip) - the stage between
`Segmenter` / `Screen` and the conditioner for recordings whose SNR is poor but whose speech is worth keeping.  The noise
spectrum of a recording is learnt from its own pauses, then every STFT frame is attenuated with a Wiener gain that is smoothed
over time and frequency.  The reference has no counterpart: its corpus arrives clean.  (`denoiser.Denoiser` is not this stage:
it subtracts one fixed, externally supplied bias spectrum - a generator's hum - from every item alike.)

    nr = NoiseReducer(22050)                                  # pauses at -40 dB, 50 ms guard, 12 dB of reduction
    r = nr(audio, audio_len)                                  # r["audio"], r["audio_len"], r["noise"], r["noise_frames"], r["flags"]

Pieces hold few pauses, so on the data side profile the *recordings*, then reduce the Segmenter's rows with the row's
recording as index (unused rows have item -1 and are copied: they are zeros):

    p = nr.profile(rec, rec_len)
    r = seg(rec, rec_len, rows=R)
    y, n = nr.apply(r["audio"], r["audio_len"], p["noise"], index=r["item"])
    nr.manifest(p, names)                                     # host rows: name, frames, noise_frames, noise_db, flag names

The frames that decide what a pause is are exactly `AudioConditioner`'s trim frames and the `Segmenter`'s.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import runtime
from .features import twiddles

__all__ = ["NoiseReducer"]

HOP, FRAME, BINS = 256, 1024, 513
KEYS = tuple(name for name, _, _ in runtime.NOISE_OUTPUTS)


def noise_tables() -> Tensor:
    """fp32 [5120] for ispk_noise_profile_f64 / ispk_noise_reduce_f32: W_2048^m as (re, im), then the periodic Hann window made in
    float64 and rounded once - denoiser.denoise_tables(), value for value (that module imports this package)."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME, dtype=np.float64) / FRAME)
    return torch.cat([twiddles().flatten(), torch.from_numpy(w.astype(np.float32))]).contiguous()


class NoiseReducer:
    """Learn each item's noise spectrum from its pauses and attenuate with a smoothed Wiener gain: four launches of
    ispk_noise_profile_f64 and one of ispk_noise_reduce_f32, with no ATen compute op, no atomics and no host read.

    nr = NoiseReducer(sample_rate, top_db=40.0, ref="max", guard_ms=50.0, min_noise_frames=8, over=2.0, reduce_db=12.0,
                      smooth_frames=2, smooth_bins=2)
    p = nr.profile(audio, audio_len, out=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride, S <= runtime.CONDITION_MAX_SAMPLES) and int64 [B] on the
                         GPU; a length n outside [0, S] counts as 0
      p["noise"]         float64 [B, 513]: the mean of |X_f[k]|^2 over the item's noise frames - the STFT frames (1024 / 256,
                         periodic Hann, the denoiser's centred framing) that lie wholly inside the item and whose trim frame
                         (AudioConditioner's: active above ref * 10^(-top_db / 10)) has no active frame within guard_frames on
                         either side; fp32 transforms, summed in float64.  Zeros without a profile
      p["noise_frames"], p["frames"]   int32 [B]: the noise frames, and all frames F = 1 + n // 256 (0 below 513 samples)
      p["flags"]         int32 [B], bits runtime.NOISE_FLAGS: 1 no_profile (noise_frames < min_noise_frames), 2 short (n < 513)
    y, n = nr.apply(audio, audio_len, noise, index=None, flags=None, out=None)
      noise              float64 [P, 513]; item b takes row index[b] (int32 [B]; None: row b)
      y                  fp32 [B, S]: X_f[k] times G_f[k], the triangular mean over smooth_frames frames and smooth_bins bins on
                         either side of the raw gain max(1 - over noise[k] / |X_f[k]|^2, g_min), g_min = 10^(-reduce_db / 20),
                         then the inverse STFT; zeros from n on.  Items below 513 samples, with a flag (int32 [B], the profile's)
                         or with a row outside [0, P) are copied bit for bit.  n is audio_len, passed through
    r = nr(audio, audio_len, out=None): both; r["audio"], r["audio_len"] and the profile's outputs.
    out: `empty_outputs(B, device, samples=S)`, allocated outside a graph capture.  An item's results depend on that item (and
    its profile row) alone - not on B, S, the row stride or what lies behind n; repeated calls and graph replays are
    bit-identical.  The host conversions are plain attributes (factor, guard_frames, g_min): a test may set small values."""

    def __init__(self, sample_rate: int, top_db: float = 40.0, ref: Union[str, float] = "max", guard_ms: float = 50.0,
                 min_noise_frames: int = 8, over: float = 2.0, reduce_db: float = 12.0, smooth_frames: int = 2,
                 smooth_bins: int = 2):
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
        if not (top_db > 0 and math.isfinite(top_db)):
            raise ValueError(f"top_db > 0, got {top_db!r}")
        if not (ref == "max" or (not isinstance(ref, str) and ref > 0 and math.isfinite(ref))):
            raise ValueError(f'ref is "max" or a positive number, got {ref!r}')
        if not (guard_ms >= 0 and math.isfinite(guard_ms)):
            raise ValueError(f"guard_ms >= 0, got {guard_ms!r}")
        if int(min_noise_frames) != min_noise_frames or min_noise_frames < 1:
            raise ValueError(f"min_noise_frames is an integer >= 1, got {min_noise_frames!r}")
        if not (over >= 0 and math.isfinite(over)):
            raise ValueError(f"over >= 0, got {over!r}")
        if not (reduce_db >= 0 and math.isfinite(reduce_db)):
            raise ValueError(f"reduce_db >= 0, got {reduce_db!r}")
        if int(smooth_frames) != smooth_frames or not 0 <= smooth_frames <= runtime.NOISE_MAX_SMOOTH_FRAMES:
            raise ValueError(f"smooth_frames is an integer in [0, {runtime.NOISE_MAX_SMOOTH_FRAMES}], got {smooth_frames!r}")
        if int(smooth_bins) != smooth_bins or not 0 <= smooth_bins <= runtime.NOISE_MAX_SMOOTH_BINS:
            raise ValueError(f"smooth_bins is an integer in [0, {runtime.NOISE_MAX_SMOOTH_BINS}], got {smooth_bins!r}")
        self.sample_rate, self.top_db = int(sample_rate), float(top_db)
        self.ref = ref if ref == "max" else float(ref)
        self.guard_ms, self.min_noise_frames = float(guard_ms), int(min_noise_frames)
        self.over, self.reduce_db = float(over), float(reduce_db)
        self.smooth_frames, self.smooth_bins = int(smooth_frames), int(smooth_bins)
        self.factor = 10.0 ** (-self.top_db / 10.0)
        self.guard_frames = int(math.ceil(self.guard_ms * self.sample_rate / 1000.0 / HOP))
        self.g_min = 10.0 ** (-self.reduce_db / 20.0)
        if self.guard_frames > runtime.NOISE_MAX_GUARD:
            raise ValueError(f"guard_ms {guard_ms!r} is {self.guard_frames} frames at {self.sample_rate} Hz: at most {runtime.NOISE_MAX_GUARD}")
        self.tables = noise_tables()
        self._on: dict = {}

    def device_tables(self, device) -> Tensor:
        """The FFT tables on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.tables.to(device)
        return t

    def empty_outputs(self, B: int, device=None, samples: Optional[int] = None) -> dict:
        """Every tensor a call writes.  "audio" and the scratch "work" depend on S: with samples=S they are made here, else the
        first call with this dict adds them (a warm-up call in front of a graph capture does)."""
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)       # noqa: E731
        out = {name: e((B, last) if last else (B,), dt) for name, dt, last in runtime.NOISE_OUTPUTS}
        if samples is not None:
            out["work"] = e((max(runtime.noise_workspace_bytes(B, int(samples)), 8),), torch.uint8)
            out["audio"] = e((B, int(samples)), torch.float32)
        return out

    def _checked(self, audio: Tensor, audio_len: Tensor) -> None:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not (audio.is_cuda and audio_len.is_cuda):
            raise runtime.IspkError("NoiseReducer needs GPU tensors; there is no CPU fallback")

    def profile(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        """The profile alone (four launches): noise, noise_frames, frames, flags."""
        self._checked(audio, audio_len)
        if audio.shape[1] > runtime.CONDITION_MAX_SAMPLES:
            raise ValueError(f"audio: at most {runtime.CONDITION_MAX_SAMPLES} samples an item, got {tuple(audio.shape)}")
        if int(self.guard_frames) != self.guard_frames or not 0 <= self.guard_frames <= runtime.NOISE_MAX_GUARD:
            raise ValueError(f"guard_frames is an integer in [0, {runtime.NOISE_MAX_GUARD}], got {self.guard_frames!r}")
        if int(self.min_noise_frames) != self.min_noise_frames or self.min_noise_frames < 1:
            raise ValueError(f"min_noise_frames is an integer >= 1, got {self.min_noise_frames!r}")
        out = {} if out is None else out
        need = runtime.noise_workspace_bytes(audio.shape[0], audio.shape[1])
        w = out.get("work")
        if w is None or w.numel() < need:
            out["work"] = torch.empty((max(need, 8),), dtype=torch.uint8, device=audio.device)
        numeric = self.ref != "max"
        r = runtime.noise_profile(audio, audio_len, self.device_tables(audio.device), self.factor, int(numeric),
                                  self.ref if numeric else 0.0, self.guard_frames, self.min_noise_frames, out)
        return {k: r[k] for k in KEYS}

    def apply(self, audio: Tensor, audio_len: Tensor, noise: Tensor, index: Optional[Tensor] = None, flags: Optional[Tensor] = None,
              out: Optional[Tensor] = None) -> tuple[Tensor, Tensor]:
        """The reduce alone (one launch) with given profiles -> (fp32 [B, S], audio_len passed through)."""
        self._checked(audio, audio_len)
        y = runtime.noise_reduce(audio, audio_len, self.device_tables(audio.device), noise, index, flags, self.over, self.g_min,
                                 self.smooth_frames, self.smooth_bins, out)
        return y, audio_len

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        out = {} if out is None else out
        r = self.profile(audio, audio_len, out)
        o = out.get("audio")
        if o is None or tuple(o.shape) != tuple(audio.shape):
            o = out["audio"] = torch.empty(tuple(audio.shape), dtype=torch.float32, device=audio.device)
        y, n = self.apply(audio, audio_len, r["noise"], None, r["flags"], o)
        r.update(audio=y, audio_len=n)
        return r

    def manifest(self, p: dict, names: Sequence[str]) -> list:
        """One dict per item, in order: name, frames, noise_frames, noise_db (10 log10 of the profile's total power sum_k
        noise[k]; None where it is zero) and the names of its flags as a tuple.  Reads back once; text, no device work."""
        host = {k: p[k].detach().cpu().tolist() for k in ("frames", "noise_frames", "flags")}
        total = p["noise"].detach().cpu().sum(dim=1).tolist()
        if len(names) != len(host["flags"]):
            raise ValueError(f"{len(host['flags'])} items: {len(names)} names given")
        rows = []
        for b, name in enumerate(names):
            rows.append({"name": name, "frames": host["frames"][b], "noise_frames": host["noise_frames"][b],
                         "noise_db": 10.0 * math.log10(total[b]) if total[b] > 0.0 else None,
                         "flags": tuple(n for n, bit in runtime.NOISE_FLAGS.items() if host["flags"][b] & bit)})
        return rows
