"""PitchTracker: probabilistic YIN (Mauch & Dixon 2014, as librosa.pyin states it) on the GPU (csrc/pyin.hip) - the pitch track
that FastPitch-family recipes outside the reference compute with `librosa.pyin`, a Python loop over frames on the host.  The
reference's own torch-yin (one threshold, an integer lag, no smoothing over time) stays the default everywhere; this is the
alternative for `AcousticFeatures(pitch_method="pyin")`, `DatasetStats` and the evaluators' F0 metrics.

    tracker = PitchTracker(22050)                             # 55 .. 880 Hz, 10 bins per semitone
    r = tracker(audio, audio_len)                             # r["f0"] Hz (0 where unvoiced), r["voiced"], r["voiced_prob"], ...
    r = tracker.normalised(mean, std)(audio, audio_len)       # also r["pitch"] = (f0 - mean) / std, the extractor's contour

Two launches, no ATen compute op, no atomics and no host read: the observation (per frame the YIN troughs of 100 thresholds under
a beta prior, binned at 10 per semitone) and the decode (Viterbi over voiced and unvoiced bins with a triangular transition
window).  Frames are the extractor's: frame t is centred where mel frame t is centred and an item has `feature_frames(n)` of
them, so the contour drops into the collator's layout.  include/ispk.h has the definition; the tables are made here in float64.
Not built: center=False framing, other hop or window sizes, fill_na modes other than 0."""
from __future__ import annotations

import copy
import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .. import runtime
from .features import twiddles

__all__ = ["PitchTracker", "beta_prior", "observation_table", "transition_table", "pitch_bins", "transition_width", "pitch_periods"]

KEYS = ("f0", "voiced", "voiced_prob", "frames", "log_prob")
TINY = float(np.finfo(np.float64).tiny)
BOLTZMANN = 2.0               # the rank prior's parameter
BETA = (2, 18)                # the threshold prior
HOP, FRAME = runtime.FEATURE_HOP, 2048


def beta_cdf(x: np.ndarray, a: int, b: int) -> np.ndarray:
    """The regularised incomplete beta function for integer a, b: the finite binomial sum sum_{j=a}^{n} C(n, j) x^j (1 - x)^(n - j),
    n = a + b - 1, in float64 (every term is non-negative; exact at 0 and 1)."""
    x = np.asarray(x, dtype=np.float64)
    n = a + b - 1
    out = np.zeros_like(x)
    for j in range(a, n + 1):
        out += math.comb(n, j) * x ** j * (1.0 - x) ** (n - j)
    return out


def beta_prior() -> np.ndarray:
    """float64 [100]: the prior of the thresholds linspace(0, 1, 101)[1:], diff(BetaCDF(2, 18)) over the 101 points."""
    return np.diff(beta_cdf(np.linspace(0.0, 1.0, runtime.PYIN_THRESHOLDS + 1), *BETA))


def observation_table() -> Tensor:
    """float64 [PYIN_TABLE_DOUBLES] as ispk_pyin_observe_f32 reads it: the thresholds, their prior, its exclusive running sum
    [101], (1 - e^-2) e^(-2 k) for k < 512 and 1 / (1 - e^(-2 N)) for N <= 512 (entry 0 unused)."""
    thr = np.linspace(0.0, 1.0, runtime.PYIN_THRESHOLDS + 1)[1:]
    prior = beta_prior()
    cum = np.concatenate([[0.0], np.cumsum(prior)])
    k = np.arange(runtime.PYIN_MAX_TROUGHS, dtype=np.float64)
    e2 = (1.0 - math.exp(-BOLTZMANN)) * np.exp(-BOLTZMANN * k)
    n = np.arange(1, runtime.PYIN_MAX_TROUGHS + 1, dtype=np.float64)
    inv = np.concatenate([[0.0], 1.0 / (1.0 - np.exp(-BOLTZMANN * n))])
    t = np.concatenate([thr, prior, cum, e2, inv])
    assert t.shape == (runtime.PYIN_TABLE_DOUBLES,)
    return torch.from_numpy(t)


def pitch_bins(f_min: float, f_max: float, bins_per_semitone: int = 10) -> int:
    """NB = floor(12 bps log2(f_max / f_min)) + 1 voiced states."""
    return int(math.floor(12 * bins_per_semitone * math.log2(f_max / f_min))) + 1


def transition_width(sample_rate: int, bins_per_semitone: int = 10, max_transition_rate: float = 35.92) -> int:
    """round(rate * 12 * hop / sr) semitones a frame, in bins, plus the centre: 51 at 22.05 kHz."""
    return int(round(max_transition_rate * 12 * HOP / sample_rate)) * bins_per_semitone + 1


def pitch_periods(sample_rate: int, f_min: float, f_max: float) -> tuple[int, int]:
    """(min_period, max_period) = (floor(sr / f_max), min(ceil(sr / f_min), 1022))."""
    return int(math.floor(sample_rate / f_max)), min(int(math.ceil(sample_rate / f_min)), runtime.PYIN_MAX_PERIOD)


def transition_table(n_bins: int, width: int, switch_prob: float = 0.01) -> Tensor:
    """float64 [width + NB + 3] as ispk_pyin_decode_f64 reads it, every log as log(p + tiny): the triangular window 1 - |k - h| /
    (h + 1), k < width, h = (width - 1) / 2; per source bin the sum of its window inside [0, NB) (its row's normaliser); stay = 1 -
    switch_prob, switch_prob; the uniform initial probability 1 / (2 NB)."""
    h = (width - 1) // 2
    tri = 1.0 - np.abs(np.arange(width, dtype=np.float64) - h) / (h + 1)
    norm = np.array([tri[max(0, h - i):min(width, n_bins - i + h)].sum() for i in range(n_bins)])
    tail = np.array([1.0 - switch_prob, switch_prob, 1.0 / (2 * n_bins)])
    return torch.from_numpy(np.log(np.concatenate([tri, norm, tail]) + TINY))


class PitchTracker:
    """pYIN pitch of zero-padded waveforms: two launches (ispk_pyin_observe_f32, ispk_pyin_decode_f64).

    tracker = PitchTracker(sample_rate, f_min=55, f_max=880, bins_per_semitone=10, switch_prob=0.01, max_transition_rate=35.92)
    r = tracker(audio, audio_len, out=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride) and int64 [B] on the GPU; nothing at or past a length is
                         read; an item below 256 samples or longer than S has no frames
      r["f0"]            fp32 [B, M], M = runtime.feature_frames(S): f_min 2^(bin / (12 bps)) Hz where voiced, 0 where unvoiced
                         (torch-yin's convention) and past the item's frames
      r["voiced"]        int32 [B, M]: 1 / 0;  r["voiced_prob"] fp32 [B, M]: the clipped sum of the frame's observation row
      r["frames"]        int64 [B]: the extractor's mel_len;  r["log_prob"] float64 [B]: the path's log-probability
      r["pitch"]         fp32 [B, M], from `tracker.normalised(mean, std)` only: (f0 - mean) / std, unvoiced frames at -mean / std,
                         0 past the item's frames - what AcousticFeatures puts into out["pitch"]
    out: `empty_outputs(B, S, device)`, allocated outside a graph capture; it also holds the observation rows ("obs" fp32
    [B, M, NB]), the path ("state" int32 [B, M], -1 past the frames) and the scratch ("work").  An item's results depend on that
    item alone; repeated calls and graph replays are bit-identical."""

    def __init__(self, sample_rate: int, f_min: float = 55.0, f_max: float = 880.0, bins_per_semitone: int = 10,
                 switch_prob: float = 0.01, max_transition_rate: float = 35.92):
        self.sample_rate, self.f_min, self.f_max = int(sample_rate), float(f_min), float(f_max)
        self.bins_per_semitone = int(bins_per_semitone)
        if not (self.sample_rate > 0 and 0.0 < self.f_min < self.f_max and 1 <= self.bins_per_semitone <= 100):
            raise ValueError(f"sample_rate {sample_rate}, f_min {f_min}, f_max {f_max}, bins_per_semitone {bins_per_semitone}: need "
                             f"0 < f_min < f_max and 1 .. 100 bins per semitone")
        if not 0.0 < switch_prob < 1.0:
            raise ValueError(f"switch_prob is in (0, 1), got {switch_prob!r}")
        self.min_period, self.max_period = pitch_periods(self.sample_rate, self.f_min, self.f_max)
        if self.min_period < 1 or self.max_period - self.min_period < 2:
            raise NotImplementedError(f"sample rate {sample_rate}, {f_min} .. {f_max} Hz: periods {self.min_period} .. "
                                      f"{self.max_period} leave fewer than three lags")
        self.n_bins = pitch_bins(self.f_min, self.f_max, self.bins_per_semitone)
        if not 1 <= self.n_bins <= runtime.PYIN_MAX_BINS:
            raise NotImplementedError(f"{f_min} .. {f_max} Hz at {bins_per_semitone} bins per semitone are {self.n_bins} bins; at most "
                                      f"{runtime.PYIN_MAX_BINS} are built")
        self.width = transition_width(self.sample_rate, self.bins_per_semitone, max_transition_rate)
        if not 1 <= self.width <= runtime.PYIN_MAX_WIDTH:
            raise NotImplementedError(f"sample rate {sample_rate}: a transition window of {self.width} bins; at most "
                                      f"{runtime.PYIN_MAX_WIDTH} are built (one backpointer byte per state)")
        self.tables = twiddles().flatten().contiguous()
        self.prior = observation_table()
        self.trans = transition_table(self.n_bins, self.width, float(switch_prob))
        self.mean: Optional[float] = None
        self.std: Optional[float] = None
        self._on: dict = {}

    def normalised(self, mean: float, std: float) -> "PitchTracker":
        """This tracker with r["pitch"] = (f0 - mean) / std on top (the extractor's normalisation; both are plain arguments of
        the launch).  Shares the tables, on the host and on every device."""
        if float(std) == 0.0:
            raise ValueError("pitch std is 0")
        t = copy.copy(self)
        t.mean, t.std = float(mean), float(std)
        return t

    def device_tables(self, device) -> tuple[Tensor, Tensor, Tensor]:
        """(twiddles, prior, trans) on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = (self.tables.to(device), self.prior.to(device), self.trans.to(device))
        return t

    def empty_outputs(self, B: int, S: int, device=None, pitch: Optional[Tensor] = None) -> dict:
        """Every tensor a call writes; `pitch` (fp32 [B, M], contiguous) is where a normalised tracker puts its contour."""
        M = runtime.feature_frames(S)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)       # noqa: E731
        out = {"obs": e((B, M, self.n_bins), torch.float32), "state": e((B, M), torch.int32), "f0": e((B, M), torch.float32),
               "voiced": e((B, M), torch.int32), "voiced_prob": e((B, M), torch.float32), "frames": e((B,), torch.int64),
               "log_prob": e((B,), torch.float64),
               "work": e((max(runtime.pyin_workspace_bytes(B, M, self.n_bins), 8),), torch.uint8)}
        if self.mean is not None or pitch is not None:
            out["pitch"] = e((B, M), torch.float32) if pitch is None else pitch
        return out

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        if audio.ndim != 2 or audio.dtype != torch.float32 or (audio.shape[1] > 1 and audio.stride(1) != 1):
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)}")
        B, S = audio.shape
        if audio_len.dtype != torch.int64 or audio_len.shape != (B,):
            raise ValueError(f"audio_len: int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not audio.is_cuda or not audio_len.is_cuda:
            raise runtime.IspkError("PitchTracker needs GPU tensors; there is no CPU fallback")
        if out is None:
            out = self.empty_outputs(B, S, audio.device)
        if self.mean is not None and out.get("pitch") is None:
            raise ValueError("out has no 'pitch' tensor: take it from this tracker's empty_outputs")
        tw, prior, trans = self.device_tables(audio.device)
        runtime.pyin_observe(audio, audio_len, tw, prior, out["obs"], out["frames"], self.min_period, self.max_period,
                             float(self.sample_rate), self.f_min, self.bins_per_semitone)
        given = {k: v for k, v in out.items() if k != "obs" and (k != "pitch" or self.mean is not None)}
        r = runtime.pyin_decode(out["obs"], out["frames"], trans, self.width, self.f_min, self.bins_per_semitone, out=given,
                                pitch_mean=self.mean if self.mean is not None else 0.0,
                                pitch_std=self.std if self.std is not None else 1.0)
        return {k: r[k] for k in KEYS + (("pitch",) if self.mean is not None else ())}
