"""Screen: is a piece fit to train on?  Clipping, dropouts, level, DC, non-finite samples and bandwidth of every item of a
padded batch, measured on the GPU (csrc/screen.hip) and folded into one word of flags per item - behind the Segmenter on the data
side, or behind a vocoder as a regression screen for synthesized audio.  The reference has no counterpart: its corpus arrives
curated.

    screen = Screen(22050, min_bandwidth_hz=7000.0)
    r = screen(audio, audio_len)                              # r["flags"] int32 [B], r["clip_runs"], r["band_bin"], r["ltas"], ...
    screen.manifest(r, names)                                 # host rows: name, the measurements, bandwidth_hz, flag names
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import torch
from torch import Tensor

from .. import runtime
from .features import twiddles

__all__ = ["Screen"]

HOP, FRAME, BINS = 256, 1024, 513
KEYS = tuple(name for name, _, _ in runtime.SCREEN_OUTPUTS)


def screen_tables() -> Tensor:
    """fp32 [5120] for ispk_screen_f64: W_2048^m as (re, im), then the extractor's fp32 periodic Hann window."""
    return torch.cat([twiddles().flatten(), torch.hann_window(FRAME, dtype=torch.float32)]).contiguous()


class Screen:
    """Measure every item and flag the unfit: four launches of ispk_screen_f64 with no ATen compute op, no atomics and no host
    read.  A non-finite sample is counted and read as 0 by everything else.

    screen = Screen(sample_rate, rail="max", rail_ratio=0.999, min_run=3, dropout_ms=5.0, band_db=60.0, min_bandwidth_hz=None,
                    max_dc=0.01, min_peak=0.0)
    r = screen(audio, audio_len, out=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride, S <= runtime.CONDITION_MAX_SAMPLES) and int64 [B] on the
                         GPU; a length n outside [0, S] counts as 0
      r["nonfinite"]     int32 [B]: NaN and Inf samples
      r["peak"]          fp32 [B]: max |x|, exact
      r["dc"], r["power"]   float64 [B]: the mean of x and of x^2, summed in float64; 0 at n = 0
      r["clip_runs"], r["clip_samples"], r["clip_longest"], r["clip_first"]   int32, int64, int64, int64 [B]: a sample is at the
                         rail when |x| >= thr > 0 with thr = the fp32 product peak * rail_ratio (rail="max") or fp32(rail); a run is a
                         maximal stretch of consecutive at-rail samples of one sign.  The runs of at least min_run samples, their
                         samples, the longest run of any length, and the start of the first counted run or -1
      r["dropout_runs"], r["dropout_samples"], r["dropout_longest"]   int32, int64, int64 [B]: the runs of x == 0 of at least
                         min_dropout_samples with a non-zero sample somewhere before and somewhere after them inside [0, n)
                         (digital silence in front and behind is padding), their samples and the longest of them
      r["ltas"]          float64 [B, 513]: the long-term average spectrum, the mean over the F = max(0, (n - 1024) // 256 + 1)
                         frames [256 f, 256 f + 1024) (periodic Hann, no padding) of |X_f[k]|^2; fp32 transforms, summed in float64
      r["band_bin"]      int32 [B]: the largest k with ltas[k] within band_db of the largest of ltas[2 .. 512] (a DC offset does not
                         set the scale); -1 when F = 0 or the spectrum is zero.  `bandwidth_hz(band_bin)` is band_bin *
                         sample_rate / 1024.  A recording upsampled from 16 kHz or decoded from MP3 has an empty top band; the
                         default of 60 dB is a trade-off - a very clean studio voice can itself fall more than 60 dB below its
                         peak near Nyquist and then reads as narrower than it is: tune band_db to the corpus
      r["flags"]         int32 [B], bits runtime.SCREEN_FLAGS: 1 clipped (clip_runs > 0), 2 narrow (min_bandwidth_hz given and
                         0 <= band_bin < min_band_bin), 4 dc (|dc| > max_dc), 8 dropout (dropout_runs > 0), 16 nonfinite, 32 quiet
                         (peak <= min_peak: true for an empty or all-zero item), 64 short (F = 0)
    out: `empty_outputs(B, device, samples=S)`, allocated outside a graph capture.  An item's results depend on that item alone
    - not on B, S, the row stride or what lies behind n; repeated calls and graph replays are bit-identical.  The host
    conversions are plain attributes (min_dropout_samples, min_band_bin (-1: no floor), band_factor): a test may set small
    values."""

    def __init__(self, sample_rate: int, rail: Union[str, float] = "max", rail_ratio: float = 0.999, min_run: int = 3,
                 dropout_ms: float = 5.0, band_db: float = 60.0, min_bandwidth_hz: Optional[float] = None, max_dc: float = 0.01,
                 min_peak: float = 0.0):
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
        if not (rail == "max" or (not isinstance(rail, str) and rail > 0 and math.isfinite(rail))):
            raise ValueError(f'rail is "max" or a positive finite level, got {rail!r}')
        if not 0 < rail_ratio <= 1:
            raise ValueError(f"0 < rail_ratio <= 1, got {rail_ratio!r}")
        if int(min_run) != min_run or min_run < 1:
            raise ValueError(f"min_run is an integer >= 1, got {min_run!r}")
        if not (dropout_ms >= 0 and math.isfinite(dropout_ms)):
            raise ValueError(f"dropout_ms >= 0, got {dropout_ms!r}")
        if not 0 < band_db <= 100:
            raise ValueError(f"0 < band_db <= 100, got {band_db!r}")
        if min_bandwidth_hz is not None and not 0 <= min_bandwidth_hz <= sample_rate / 2:
            raise ValueError(f"min_bandwidth_hz is None or in [0, sample_rate / 2], got {min_bandwidth_hz!r}")
        for name, v in (("max_dc", max_dc), ("min_peak", min_peak)):
            if not (v >= 0 and math.isfinite(v)):
                raise ValueError(f"{name} >= 0, got {v!r}")
        self.sample_rate = int(sample_rate)
        self.rail = rail if rail == "max" else float(rail)
        self.rail_ratio, self.min_run, self.dropout_ms = float(rail_ratio), int(min_run), float(dropout_ms)
        self.band_db = float(band_db)
        self.min_bandwidth_hz = None if min_bandwidth_hz is None else float(min_bandwidth_hz)
        self.max_dc, self.min_peak = float(max_dc), float(min_peak)
        self.band_factor = 10.0 ** (-self.band_db / 10.0)
        self.min_dropout_samples = max(1, int(round(self.dropout_ms * self.sample_rate / 1000.0)))
        # band_bin < min_band_bin exactly when band_bin * sample_rate / 1024 < min_bandwidth_hz
        self.min_band_bin = -1 if self.min_bandwidth_hz is None else int(math.ceil(self.min_bandwidth_hz * FRAME / self.sample_rate))
        self.tables = screen_tables()
        self._on: dict = {}

    def bandwidth_hz(self, band_bin):
        """band_bin * sample_rate / 1024 (a number or a tensor; -1 stays negative: no spectrum)."""
        return band_bin * (self.sample_rate / FRAME)

    def device_tables(self, device) -> Tensor:
        """The FFT tables on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.tables.to(device)
        return t

    def empty_outputs(self, B: int, device=None, samples: Optional[int] = None) -> dict:
        """Every tensor a call writes.  The scratch "work" depends on S: with samples=S it is made here, else the first call with
        this dict adds it (a warm-up call in front of a graph capture does)."""
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)       # noqa: E731
        out = {name: e((B, last) if last else (B,), dt) for name, dt, last in runtime.SCREEN_OUTPUTS}
        if samples is not None:
            out["work"] = e((max(runtime.screen_workspace_bytes(B, int(samples)), 8),), torch.uint8)
        return out

    def _checked(self, audio: Tensor, audio_len: Tensor) -> None:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        if audio.shape[1] > runtime.CONDITION_MAX_SAMPLES:
            raise ValueError(f"audio: at most {runtime.CONDITION_MAX_SAMPLES} samples an item, got {tuple(audio.shape)}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not (audio.is_cuda and audio_len.is_cuda):
            raise runtime.IspkError("Screen needs GPU tensors; there is no CPU fallback")
        if int(self.min_run) != self.min_run or self.min_run < 1:
            raise ValueError(f"min_run is an integer >= 1, got {self.min_run!r}")
        if int(self.min_dropout_samples) != self.min_dropout_samples or self.min_dropout_samples < 1:
            raise ValueError(f"min_dropout_samples is an integer >= 1, got {self.min_dropout_samples!r}")
        if int(self.min_band_bin) != self.min_band_bin or not -1 <= self.min_band_bin <= BINS:
            raise ValueError(f"min_band_bin is an integer in [-1, {BINS}], got {self.min_band_bin!r}")

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None, parts: int = 3) -> dict:
        """parts: 1 levels and runs only, 2 the spectrum only (tools/time_screen.py times them apart); 3 is the screen."""
        self._checked(audio, audio_len)
        out = {} if out is None else out
        need = runtime.screen_workspace_bytes(audio.shape[0], audio.shape[1])
        w = out.get("work")
        if w is None or w.numel() < need:
            out["work"] = torch.empty((max(need, 8),), dtype=torch.uint8, device=audio.device)
        numeric = self.rail != "max"
        r = runtime.screen(audio, audio_len, self.device_tables(audio.device), int(numeric), self.rail if numeric else 0.0,
                           self.rail_ratio, self.min_run, self.min_dropout_samples, self.band_factor, self.min_band_bin, self.max_dc,
                           self.min_peak, out, parts)
        return {k: r[k] for k in KEYS}

    def manifest(self, r: dict, names: Sequence[str]) -> list:
        """One dict per item, in order: name, every measurement but the spectrum as a Python number, bandwidth_hz (None without a
        spectrum) and the names of its flags as a tuple.  Reads back once; text, no device work."""
        host = {k: r[k].detach().cpu().tolist() for k in KEYS if k != "ltas"}
        if len(names) != len(host["flags"]):
            raise ValueError(f"{len(host['flags'])} items: {len(names)} names given")
        rows = []
        for b, name in enumerate(names):
            row = {"name": name}
            row.update({k: host[k][b] for k in host if k != "flags"})
            row["bandwidth_hz"] = None if row["band_bin"] < 0 else self.bandwidth_hz(row["band_bin"])
            row["flags"] = tuple(n for n, bit in runtime.SCREEN_FLAGS.items() if host["flags"][b] & bit)
            rows.append(row)
        return rows
