"""TimeStretch and PitchShift: tempo without pitch, and pitch without tempo, on the GPU (csrc/stretch.hip) - the waveform
operation that augmentation of a small fine-tuning set and the last touch on finished audio otherwise leave the device for
(librosa.effects.time_stretch / pitch_shift).  The reference has no counterpart.  It is the plain phase vocoder that torchaudio
and librosa ship (no phase locking, no transient preservation) on the denoiser's 1024 / 256 STFT.

    ts = TimeStretch(1.25)                                    # 1.25 times as fast, 1 / 1.25 as long
    r = ts(audio, audio_len)                                  # r["audio"], r["audio_len"], r["wanted"], r["flags"]

    rate = torch.empty(B, dtype=torch.float64, device=dev)    # one rate per item, device data: one capture serves every draw
    out = ts.empty_outputs(B, dev, samples=2 * S + 1)
    r = ts(audio, audio_len, rate=rate, out=out)

    ps = PitchShift(22050, steps=1)                           # one semitone up: the pitch times 18 / 17
    r = ps(audio, audio_len)                                  # the same length, within one sample
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import torch
from torch import Tensor

from .. import runtime
from .noise import noise_tables
from .resample import Resampler

__all__ = ["TimeStretch", "PitchShift", "nearest_ratio"]

KEYS = ("audio", "audio_len", "wanted", "flags")


def _rate_ok(rate) -> bool:
    return isinstance(rate, (int, float)) and not isinstance(rate, bool) and runtime.STRETCH_RATES[0] <= rate <= runtime.STRETCH_RATES[1]


class TimeStretch:
    """The phase vocoder: three launches of ispk_stretch_f32, with no ATen compute op, no atomics and no host read.

    ts = TimeStretch(rate=None)
    r = ts(audio, audio_len, rate=None, out=None, out_samples=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride, 1 <= S <= runtime.CONDITION_MAX_SAMPLES) and int64 [B] on
                         the GPU; a length n outside [0, S] counts as 0
      rate               a float in [0.5, 2] (the call's, else the constructor's), or a float64 [B] tensor on the GPU with one
                         rate per item.  Output frame j sits at analysis time j rate: the magnitudes of the analysis frames
                         floor(j rate) and the next are interpolated, and the phase of every bin advances by their phase
                         difference (include/ispk.h has the definition).  Phases are unit phasors multiplied in float64
      r["audio"]         fp32 [B, out_samples]: the item's round(n / rate) samples (half to even), cut at out_samples; zeros behind.
                         With a float rate out_samples defaults to ceil(S / rate) + 1, which holds every item whole; with a
                         tensor it is required (or taken from out["audio"])
      r["audio_len"]     int64 [B]: min(wanted, out_samples);  r["wanted"] int64 [B]: round(n / rate)
      r["flags"]         int32 [B], bits runtime.STRETCH_FLAGS: 1 short (n < 513: copied), 2 truncated (wanted > out_samples),
                         4 bad_rate (a device rate that is NaN or outside [0.5, 2]: copied)
    out: `empty_outputs(B, device, samples=out_samples)`, allocated outside a graph capture.  An item's results depend on its
    samples, n and rate alone - not on B, S, the row stride, out_samples (at least wanted), its neighbours or what lies behind
    n; repeated calls and graph replays are bit-identical.  Rate 1 is the STFT round trip: the input within fp32 rounding."""

    def __init__(self, rate: Optional[float] = None):
        if rate is not None and not _rate_ok(rate):
            raise ValueError(f"rate is a number in [{runtime.STRETCH_RATES[0]}, {runtime.STRETCH_RATES[1]}] or None, got {rate!r}")
        self.rate = None if rate is None else float(rate)
        self.tables = noise_tables()
        self._on: dict = {}

    def device_tables(self, device) -> Tensor:
        """The FFT tables on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.tables.to(device)
        return t

    @staticmethod
    def out_samples(S: int, rate: float) -> int:
        """ceil(S / rate) + 1: holds round(n / rate) for every n <= S."""
        return int(math.ceil(S / float(rate))) + 1

    def empty_outputs(self, B: int, device=None, samples: Optional[int] = None) -> dict:
        """Every tensor a call writes.  "audio" and the scratch "work" depend on out_samples: with samples=out_samples they are
        made here, else the first call with this dict adds them (a warm-up call in front of a graph capture does)."""
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)       # noqa: E731
        out = {"audio_len": e((B,), torch.int64), "wanted": e((B,), torch.int64), "flags": e((B,), torch.int32)}
        if samples is not None:
            if int(samples) != samples or not 1 <= samples <= runtime.CONDITION_MAX_SAMPLES:
                raise ValueError(f"samples is an integer in [1, {runtime.CONDITION_MAX_SAMPLES}], got {samples!r}")
            out["work"] = e((max(runtime.stretch_workspace_bytes(B, 0, int(samples)), 8),), torch.uint8)
            out["audio"] = e((B, int(samples)), torch.float32)
        return out

    def __call__(self, audio: Tensor, audio_len: Tensor, rate: Union[None, float, Tensor] = None, out: Optional[dict] = None,
                 out_samples: Optional[int] = None) -> dict:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1 or audio.shape[1] < 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S and S >= 1, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        B, S = audio.shape
        if audio_len.dtype != torch.int64 or audio_len.shape != (B,):
            raise ValueError(f"audio_len: int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        rate = self.rate if rate is None else rate
        if rate is None:
            raise ValueError("no rate: give one to the constructor or to the call")
        per_item = isinstance(rate, Tensor)
        if per_item:
            if rate.dtype != torch.float64 or rate.shape != (B,) or not rate.is_contiguous():
                raise ValueError(f"rate: a float or a contiguous float64 [{B}] tensor, got {rate.dtype} {tuple(rate.shape)}")
        elif not _rate_ok(rate):
            raise ValueError(f"rate is a number in [{runtime.STRETCH_RATES[0]}, {runtime.STRETCH_RATES[1]}], got {rate!r}")
        if not (audio.is_cuda and audio_len.is_cuda and (not per_item or rate.is_cuda)):
            raise runtime.IspkError("TimeStretch needs GPU tensors; there is no CPU fallback")
        out = {} if out is None else out
        o = out.get("audio")
        if out_samples is None:
            if o is not None:
                out_samples = o.shape[-1]
            elif per_item:
                raise ValueError("a rate per item needs out_samples (or out['audio']): the lengths are device data")
            else:
                out_samples = self.out_samples(S, rate)
        if int(out_samples) != out_samples or not 1 <= out_samples <= runtime.CONDITION_MAX_SAMPLES:
            raise ValueError(f"out_samples is an integer in [1, {runtime.CONDITION_MAX_SAMPLES}], got {out_samples!r}")
        out_samples = int(out_samples)
        if o is None or tuple(o.shape) != (B, out_samples):
            if o is not None:
                raise ValueError(f"out['audio']: fp32 [{B}, {out_samples}], got {tuple(o.shape)}")
            o = out["audio"] = torch.empty((B, out_samples), dtype=torch.float32, device=audio.device)
        for k, dt in (("audio_len", torch.int64), ("wanted", torch.int64), ("flags", torch.int32)):
            if out.get(k) is None:
                out[k] = torch.empty((B,), dtype=dt, device=audio.device)
        need = runtime.stretch_workspace_bytes(B, S, out_samples)
        w = out.get("work")
        if w is None or w.numel() < need:
            out["work"] = torch.empty((max(need, 8),), dtype=torch.uint8, device=audio.device)
        runtime.stretch(audio, audio_len, self.device_tables(audio.device), rate if per_item else float(rate), o, out["audio_len"],
                        out["wanted"], out["flags"], out["work"])
        return {k: out[k] for k in KEYS}

    def manifest(self, r: dict, names: Sequence[str], audio_len: Optional[Tensor] = None) -> list:
        """One dict per item, in order: name, samples_in (the input lengths, where `audio_len` is given; else None), samples_out,
        wanted and the names of its flags as a tuple.  Reads back once; text, no device work."""
        host = {k: r[k].detach().cpu().tolist() for k in ("audio_len", "wanted", "flags")}
        n_in = None if audio_len is None else audio_len.detach().cpu().tolist()
        if len(names) != len(host["flags"]):
            raise ValueError(f"{len(host['flags'])} items: {len(names)} names given")
        return [{"name": name, "samples_in": None if n_in is None else n_in[b], "samples_out": host["audio_len"][b],
                 "wanted": host["wanted"][b],
                 "flags": tuple(n for n, bit in runtime.STRETCH_FLAGS.items() if host["flags"][b] & bit)}
                for b, name in enumerate(names)]


def nearest_ratio(target: float, max_den: int) -> tuple[int, int]:
    """(p, q) in lowest terms with q <= max_den and p / q nearest `target` (the smaller q on a tie)."""
    best = None
    for q in range(1, int(max_den) + 1):
        p = max(1, int(round(target * q)))
        err = abs(p / q - target)
        if best is None or err < best[0]:
            best = (err, p, q)
    g = math.gcd(best[1], best[2])
    return best[1] // g, best[2] // g


class PitchShift:
    """Pitch without tempo: `TimeStretch` at rate q / p, then `Resampler(p, q)` - the pitch is multiplied by p / q.  Two
    existing-style stages, four launches, no kernel of its own.

    ps = PitchShift(sample_rate, steps=None, ratio=None, max_den=32)
      steps     semitones (a number); the ratio is the fraction nearest 2^(steps / 12) with a denominator of at most max_den
      ratio     (p, q) given outright, positive integers, reduced; one of steps and ratio
      .ratio, .cents_error   (p, q) in lowest terms, and 1200 log2((p / q) / 2^(steps / 12)) (0 with ratio=)
    q / p must lie in [0.5, 2] (an octave either way); if Resampler refuses the pair (its tap table lives in LDS), the
    constructor passes its NotImplementedError on.
    r = ps(audio, audio_len, out=None): r["audio"] fp32 [B, ceil(q (ceil(S p / q) + 1) / p)], r["audio_len"] int64 [B] - the
    resampler's own lengths, ceil(q round(n p / q) / p): within one sample of n -, and the stretch's r["wanted"], r["flags"],
    r["stretched"], r["stretched_len"].  out: `empty_outputs(B, S, device)`, so that the pair captures."""

    def __init__(self, sample_rate: int, steps: Optional[float] = None, ratio: Optional[tuple] = None, max_den: int = 32):
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
        if (steps is None) == (ratio is None):
            raise ValueError("give one of steps and ratio")
        if int(max_den) != max_den or max_den < 1:
            raise ValueError(f"max_den is an integer >= 1, got {max_den!r}")
        if ratio is not None:
            if len(ratio) != 2 or any(int(v) != v or v <= 0 for v in ratio):
                raise ValueError(f"ratio is a pair of positive integers, got {ratio!r}")
            g = math.gcd(int(ratio[0]), int(ratio[1]))
            p, q = int(ratio[0]) // g, int(ratio[1]) // g
            target = p / q
        else:
            if not (isinstance(steps, (int, float)) and math.isfinite(steps)):
                raise ValueError(f"steps is a finite number of semitones, got {steps!r}")
            target = 2.0 ** (float(steps) / 12.0)
            p, q = nearest_ratio(target, int(max_den))
        if not runtime.STRETCH_RATES[0] <= q / p <= runtime.STRETCH_RATES[1]:
            raise ValueError(f"a pitch ratio of {p} / {q} needs a stretch by {q} / {p}, outside [{runtime.STRETCH_RATES[0]}, "
                             f"{runtime.STRETCH_RATES[1]}]")
        self.sample_rate, self.steps, self.max_den = int(sample_rate), steps, int(max_den)
        self.ratio = (p, q)
        self.cents_error = 1200.0 * math.log2((p / q) / target)
        self.stretch = TimeStretch(q / p)
        self.resampler = Resampler(p, q)

    def device_tables(self, device):
        return self.stretch.device_tables(device), self.resampler.device_tables(device)

    def stretched_samples(self, S: int) -> int:
        return TimeStretch.out_samples(S, self.stretch.rate)

    def empty_outputs(self, B: int, S: int, device) -> dict:
        """Both stages' outputs for input rows of S samples."""
        mid = self.stretched_samples(S)
        st = self.stretch.empty_outputs(B, device, samples=mid)
        a, ln = self.resampler.empty_outputs(B, mid, device)
        return {"stretch": st, "audio": a, "audio_len": ln}

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        if audio.ndim != 2:
            raise ValueError(f"PitchShift takes mono fp32 [B, S], got {tuple(audio.shape)}")
        if out is None:
            if not audio.is_cuda:
                raise runtime.IspkError("PitchShift needs GPU tensors; there is no CPU fallback")
            out = self.empty_outputs(audio.shape[0], audio.shape[1], audio.device)
        s = self.stretch(audio, audio_len, out=out["stretch"], out_samples=self.stretched_samples(audio.shape[1]))
        a, ln = self.resampler(s["audio"], s["audio_len"], out=(out["audio"], out["audio_len"]))
        return {"audio": a, "audio_len": ln, "wanted": s["wanted"], "flags": s["flags"], "stretched": s["audio"],
                "stretched_len": s["audio_len"]}
