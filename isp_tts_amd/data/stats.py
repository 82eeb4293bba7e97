"""The dataset statistics pass on the device: `AcousticDataset.compute_stats` (data/dataset.py:174-221 of the reference) with
`remove_outliers` (data/functions.py:27-32) as a launch pair of ispk_feature_stats_f64 (csrc/audio.hip) per batch.

Per utterance and feature the values x[b, :mel_len[b]] (the pitch's trailing 0 of dataset.py:152 included, as in the
reference's `inputs.pitch`) lose their IQR outliers - kept: p25 - 1.5 IQR < v < p75 + 1.5 IQR, strictly, with the
linear-interpolation quantiles of torch.quantile - and, for pitch, everything that is not > 0.  What follows from the rule:
an utterance with 75 % or more unvoiced frames has IQR 0 at 0 and contributes no pitch; a constant energy, a single frame,
an utterance holding a NaN, and mel_len 0 contribute nothing.  The kept values' count, mean, M2, min and max are pooled
across utterances in float64 (the reference pools in fp32 with E[x^2] - mean^2).  Nothing is read back before `result()`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
from torch import Tensor

from .. import runtime


@dataclass
class FeatureStats:
    min: float
    max: float
    mean: float
    std: float
    count: int

    def to_dict(self) -> dict:
        return {"min": float(self.min), "max": float(self.max), "mean": float(self.mean), "std": float(self.std)}


@dataclass
class DatasetStatsResult:
    pitch: FeatureStats
    energy: FeatureStats

    @property
    def counts(self) -> dict:
        return {"pitch": self.pitch.count, "energy": self.energy.count}

    def to_dict(self) -> dict:
        """The reference's stats.json layout; AcousticFeatures.from_config takes it under dataset.stats."""
        return {"pitch": self.pitch.to_dict(), "energy": self.energy.to_dict()}


class DatasetStats:
    """stats = DatasetStats(device);  stats.update(pitch, energy, mel_len) per batch;  stats.result().
      pitch, energy  fp32 [B, M] on the GPU (unit stride on M), M <= 4096: what AcousticFeatures(pitch_mean=0, pitch_std=1)
                     returns, so pitch in Hz with 0 on unvoiced frames
      mel_len        int64 [B] on the GPU; a length below 0 or above M counts as 0
    `partials` holds the last batch's float64 [B, 2, 5] (count, mean, M2, min, max) per (utterance, feature); `state` the
    pooled float64 [2, 5].  update() is a launch pair with no ATen compute op and no host read, so it can be captured."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise runtime.IspkError("DatasetStats needs a GPU device; there is no CPU fallback")
        self.state = torch.empty((2, 5), dtype=torch.float64, device=self.device)
        self.partials = None
        self.reset()

    def reset(self) -> None:
        runtime.feature_stats(None, None, None, None, self.state, reset=True)

    def update(self, pitch: Tensor, energy: Tensor, mel_len: Tensor) -> None:
        if pitch.ndim != 2 or pitch.shape[1] > runtime.STATS_MAX_FRAMES:
            raise ValueError(f"pitch: fp32 [B, M] with M <= {runtime.STATS_MAX_FRAMES}, got {tuple(pitch.shape)}")
        B = pitch.shape[0]
        if self.partials is None or self.partials.shape[0] != B:
            self.partials = torch.empty((B, 2, 5), dtype=torch.float64, device=self.device)
        if B:
            runtime.feature_stats(pitch, energy, mel_len, self.partials, self.state)

    def result(self) -> DatasetStatsResult:
        """Reads the state (the one host read).  ValueError for a feature with no kept value."""
        s = self.state.cpu().tolist()
        out = []
        for name, (count, mean, m2, mn, mx) in zip(("pitch", "energy"), s):
            if count <= 0:
                raise ValueError(f"no {name} value was kept: the statistics are undefined")
            out.append(FeatureStats(min=mn, max=mx, mean=mean, std=math.sqrt(m2 / count), count=int(count)))
        return DatasetStatsResult(*out)
