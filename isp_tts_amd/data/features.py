"""The acoustic dataset's per-sample features from waveforms, batched on the GPU: what `AcousticDataset.__getitem__`
(data/dataset.py:131-171 of the reference) computes on the CPU with `SpectrogramProvider`, `MelScaleProvider`,
`EnergyProvider` and the torch-yin `PitchProvider` (data/providers.py, data/pitch.py), followed by the pitch pad of
dataset.py:152 and `AcousticCollator` (data/collator.py:27-95).

`AcousticFeatures(audio, audio_len)` is ONE launch of ispk_audio_features_f32 (csrc/features.hip): no ATen compute op and
no host read, so it can run inside a captured training step (train.GraphedTrainStep(..., features=)).  Per utterance the
result is the reference's providers on that utterance alone, unpadded, then collated.  The filterbank the reference takes
from torchaudio.functional.melscale_fbanks is restated below from torchaudio's documented definition (torchaudio is not a
dependency).  Decoding stays on the host (AudioProvider); data.Resampler resamples on the device.
"""
from __future__ import annotations

import math
import os
from collections.abc import Mapping
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import runtime

N_FFT = 1024
HOP = runtime.FEATURE_HOP
PAD = int((N_FFT - HOP) / 2)                     # SpectrogramProvider / PitchProvider default pad: 384


def _hz_to_mel_slaney(f: np.ndarray) -> np.ndarray:
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz_slaney(m: np.ndarray) -> np.ndarray:
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int, norm: Optional[str] = "slaney",
                    mel_scale: str = "slaney") -> Tensor:
    """torchaudio.functional.melscale_fbanks for mel_scale="slaney": fp32 [n_freqs, n_mels] (spec^T @ fb = the mel spectrum).
    Bin k sits at linspace(0, sample_rate // 2, n_freqs)[k]; n_mels + 2 points equally spaced on the slaney mel scale
    (linear below 1 kHz, logarithmic above) from f_min to f_max; filter m is the triangle over points m, m + 1, m + 2, clipped
    at zero; norm="slaney" scales it by 2 / (f_{m+2} - f_m) (constant area).  Evaluated in float64 and rounded once."""
    if mel_scale != "slaney" or norm not in (None, "slaney"):
        raise NotImplementedError("only the slaney mel scale, with slaney or no normalisation, is built (the recipes' choice)")
    all_freqs = np.linspace(0.0, float(sample_rate // 2), n_freqs)
    m_pts = np.linspace(_hz_to_mel_slaney(f_min), _hz_to_mel_slaney(f_max), n_mels + 2)
    f_pts = _mel_to_hz_slaney(m_pts)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == "slaney":
        fb *= (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]
    return torch.from_numpy(fb.astype(np.float32))


def pack_filterbank(fb: Tensor) -> tuple[Tensor, Tensor]:
    """fp32 [n_freqs, n_mels] -> (weights fp32 [nnz], index int32 [2 n_mels + 1]) as ispk_audio_features_f32 reads them:
    first bin of each filter's contiguous non-zero range, then the offsets of each filter's weights."""
    n_mels = fb.shape[1]
    lo, off, w = [], [0], []
    for m in range(n_mels):
        nz = torch.nonzero(fb[:, m] != 0).flatten().tolist()
        a, b = (nz[0], nz[-1] + 1) if nz else (0, 0)
        assert b - a == len(nz), "a filter's non-zero bins are not contiguous"
        lo.append(a)
        w.append(fb[a:b, m])
        off.append(off[-1] + b - a)
    return torch.cat(w) if w else torch.zeros(0), torch.tensor(lo + off, dtype=torch.int32)


def twiddles() -> Tensor:
    """fp32 [2048, 2]: exp(-2 pi i m / 2048) as (re, im), evaluated in float64 and rounded once."""
    a = 2.0 * np.pi * np.arange(2048, dtype=np.float64) / 2048.0
    return torch.from_numpy(np.stack([np.cos(a), -np.sin(a)], axis=1).astype(np.float32))


def yin_lags(sample_rate: int, win_length: int = N_FFT, f_max: float = 800) -> tuple[int, int]:
    """(tau_min, tau_max) of torch-yin as PitchProvider calls it: f_min is overridden to 2 int(sr / win_length)
    (providers.py:300); pitch.py:44-45 takes int(sr / f_max) and int(sr / f_min)."""
    return int(sample_rate / f_max), int(sample_rate / (2 * int(sample_rate / win_length)))


def pitch_frames(samples: int, tau_max: int) -> int:
    """YIN frames of an utterance (pitch.py:62-66 on the 384-padded signal): (max(S + 768, 2 tau_max) - 2 tau_max) // 256 + 1."""
    fl = 2 * tau_max
    return (max(samples + 2 * PAD, fl) - fl) // HOP + 1


def _resolve(value, root):
    """An OmegaConf-style `${dataset.a.b}` reference of the recipe, looked up in the dataset section `root`."""
    if isinstance(value, str) and value.startswith("${") and value.endswith("}"):
        path = value[2:-1].split(".")
        if path[0] == "dataset":
            path = path[1:]
        node = root
        for p in path:
            node = node[p]
        return _resolve(node, root)
    return value


def _section(cfg, name: str, root) -> Optional[dict]:
    if cfg is None or name not in cfg or cfg[name] is None:
        return None
    sec = {k: _resolve(v, root) for k, v in dict(cfg[name]).items()}
    if sec.pop("_disable_", False):
        return None
    return sec


def _pitch_stats(stats) -> Mapping:
    """{mean, std} of the pitch from the dataset's `stats` as dataset.py:115-127 takes it: absent, a mapping (a dict or
    OmegaConf's DictConfig) of {pitch: {mean, std}}, or an AcousticDatasetStats-like object.  A stats file is refused."""
    if stats is None:
        return {}
    if isinstance(stats, Mapping):
        return stats.get("pitch") or {}
    if isinstance(stats, (str, os.PathLike)):
        raise NotImplementedError("dataset stats from a file: pass the values (stats.pitch.mean / std)")
    pitch = stats.pitch
    return {"mean": pitch.mean, "std": pitch.std}


class AcousticFeatures:
    """Batched log-mel, energy and torch-yin pitch of zero-padded waveforms.

    feats = AcousticFeatures.from_config(recipe["dataset"]);  out = feats(audio, audio_len)
      audio      fp32 [B, S] on the GPU (unit stride on S), zero-padded or not: nothing at or past audio_len[b] is read
      audio_len  int64 [B] on the GPU
      out        {"mel": fp32 [B, n_mels, M], "mel_len": int64 [B], "pitch": fp32 [B, M] or None, "energy": fp32 [B, M] or None},
                 M = (S + 768 - 1024) // 256 + 1 (0 below 256 samples), zeros past each mel_len; an utterance below 256
                 samples (where the reference's torch.stft raises) or longer than S gets mel_len 0 and zero rows.
    Pitch is normalised with the dataset stats ((hz - mean) / std, unvoiced frames -mean / std) and 0 past its own frame
    count, as dataset.py:151-152 leaves it.
    pitch_method="pyin": the contour is data.PitchTracker's (pitch_f_min .. pitch_f_max Hz, csrc/pyin.hip) instead, normalised
    the same way, one value per mel frame; the extractor's launch then computes no pitch and two launches follow it.  The
    tracker's own tensors (f0 in Hz, voiced flags, ...) are in out["pyin"]."""

    PITCH_METHODS = ("torch-yin", "pyin")

    def __init__(self, sample_rate: int = 22050, n_mels: int = 80, f_min: float = 0.0, f_max: Optional[float] = 8000.0,
                 pitch: bool = True, pitch_f_max: float = 800, pitch_threshold: float = 0.15, pitch_mean: float = 0.0,
                 pitch_std: float = 1.0, energy: bool = True, mel_sample_rate: Optional[int] = None,
                 pitch_method: str = "torch-yin", pitch_f_min: float = 55.0):
        self.sample_rate = int(sample_rate)
        mel_sr = int(mel_sample_rate if mel_sample_rate is not None else sample_rate)
        self.n_mels = int(n_mels)
        if not 1 <= self.n_mels <= 128:
            raise NotImplementedError(f"n_mels={n_mels}: 1 .. 128 mel channels are built")
        if pitch_method not in self.PITCH_METHODS:
            raise NotImplementedError(f"pitch method {pitch_method!r}: only torch-yin is built")
        self.pitch, self.energy = bool(pitch), bool(energy)
        self.pitch_method, self.tracker = pitch_method, None
        self.threshold, self.pitch_mean, self.pitch_std = float(pitch_threshold), float(pitch_mean), float(pitch_std)
        self.tau_min, self.tau_max = yin_lags(self.sample_rate, N_FFT, pitch_f_max)
        if self.pitch and pitch_method == "pyin":
            from .pitch import PitchTracker
            self.tracker = PitchTracker(self.sample_rate, f_min=pitch_f_min, f_max=pitch_f_max)
            if self.pitch_std == 0.0:
                raise ValueError("pitch std is 0")
        elif self.pitch:
            if int(HOP / self.sample_rate * self.sample_rate) != HOP:        # providers.py:298 and pitch.py:47
                raise NotImplementedError(f"sample rate {sample_rate}: torch-yin's frame stride would not be {HOP}")
            if not (1 <= self.tau_min < self.tau_max - 1 and 2 * self.tau_max >= N_FFT and 3 * self.tau_max <= 2048):
                raise NotImplementedError(f"sample rate {sample_rate}, f_max {pitch_f_max}: lags {self.tau_min} .. "
                                          f"{self.tau_max} need 1 <= tau_min < tau_max - 1 and 512 <= tau_max <= 682 (a "
                                          f"wrap-free 2048-point autocorrelation)")
            if self.pitch_std == 0.0:
                raise ValueError("pitch std is 0")
        self.fb = melscale_fbanks(N_FFT // 2 + 1, float(f_min), float(f_max if f_max is not None else mel_sr // 2),
                                  self.n_mels, mel_sr, "slaney", "slaney")
        weights, self.fb_index = pack_filterbank(self.fb)
        window = torch.hann_window(N_FFT, dtype=torch.float32)              # the Spectrogram's window_fn (periodic)
        self.tables = torch.cat([twiddles().flatten(), window, weights]).contiguous()
        self._on: dict = {}

    @classmethod
    def from_config(cls, dataset) -> "AcousticFeatures":
        """From the recipe's `dataset` section (recipes/acoustic/core.yaml): audio.sample_rate, spec, mel_scale, pitch,
        energy, stats, pitch_from_disk, with `_disable_` and `${dataset...}` references as the reference resolves them.
        Options the recipes never enable raise NotImplementedError."""
        d = dict(dataset)
        if d.get("pitch_from_disk", False):
            raise NotImplementedError("pitch_from_disk: pitch is computed from the waveform here")
        sr = int(_resolve(d["audio"]["sample_rate"], d))
        spec = _section(d, "spec", d) or {}
        if int(spec.get("n_fft", N_FFT)) != N_FFT or int(spec.get("win_length", N_FFT)) != N_FFT:
            raise NotImplementedError("n_fft / win_length other than 1024 are not built")
        if int(spec.get("hop_length", HOP)) != HOP:
            raise NotImplementedError("hop_length other than 256 is not built")
        if spec.get("pad") is not None and int(spec["pad"]) != PAD:
            raise NotImplementedError("a spectrogram pad other than (n_fft - hop) / 2 is not built")
        if spec.get("center", False):
            raise NotImplementedError("center=True is not built (the recipes' spectrogram is center=False)")
        if spec.get("power", 1.0) is None or float(spec.get("power", 1.0)) != 1.0:
            raise NotImplementedError("only the magnitude spectrogram (power=1) is built")
        if spec.get("normalized", False):
            raise NotImplementedError("normalized spectrograms are not built")
        ms = _section(d, "mel_scale", d)
        if ms is None:
            raise ValueError("the dataset has no mel_scale section")
        if int(ms.get("n_fft", N_FFT)) != N_FFT:
            raise NotImplementedError("mel_scale.n_fft other than 1024 is not built")
        if ms.get("mel_scale", "slaney") != "slaney" or ms.get("norm", "slaney") != "slaney":
            raise NotImplementedError("only the slaney mel scale with slaney normalisation is built (the recipes' choice)")
        pitch = _section(d, "pitch", d)
        kw = {}
        if pitch is not None:
            if pitch.get("method", "torch-yin") not in cls.PITCH_METHODS:
                raise NotImplementedError(f"pitch method {pitch['method']!r}: only torch-yin is built")
            if pitch.get("method", "torch-yin") == "pyin":
                kw.update(pitch_method="pyin", pitch_f_min=float(pitch.get("f_min", 55.0)))
            if int(pitch.get("hop_length", HOP)) != HOP or int(pitch.get("win_length", N_FFT)) != N_FFT:
                raise NotImplementedError("pitch hop_length / win_length other than 256 / 1024 are not built")
            if pitch.get("pad") is not None and int(pitch["pad"]) != PAD:
                raise NotImplementedError("a pitch pad other than (win_length - hop) / 2 is not built")
            if int(pitch.get("sample_rate", sr)) != sr:
                raise NotImplementedError("a pitch sample rate other than the audio's is not built")
            kw.update(pitch_f_max=float(pitch.get("f_max", 800)), pitch_threshold=float(pitch.get("threshold", 0.15)))
        pstats = _pitch_stats(d.get("stats"))
        return cls(sample_rate=sr, n_mels=int(ms.get("n_mels", 80)), f_min=float(ms.get("f_min", 0.0)),
                   f_max=None if ms.get("f_max", 8000.0) is None else float(ms.get("f_max", 8000.0)), pitch=pitch is not None,
                   pitch_mean=float(pstats.get("mean", 0.0)), pitch_std=float(pstats.get("std", 1.0)),
                   energy=_section(d, "energy", d) is not None, mel_sample_rate=int(ms.get("sample_rate", sr)), **kw)

    def set_pitch_stats(self, mean: float, std: float) -> None:
        """The dataset's pitch mean / std (e.g. DatasetStats.result().pitch) for the normalisation.  Both are plain arguments
        of the launch: no table is rebuilt.  (A graph captured earlier keeps the values it was captured with.)"""
        if float(std) == 0.0:
            raise ValueError("pitch std is 0")
        self.pitch_mean, self.pitch_std = float(mean), float(std)

    def device_tables(self, device) -> tuple[Tensor, Tensor]:
        """(tables, fb_index) on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = (self.tables.to(device), self.fb_index.to(device))
            if self.tracker is not None:
                self.tracker.device_tables(device)
        return t

    def empty_outputs(self, B: int, S: int, device) -> dict:
        M = runtime.feature_frames(S)
        f32 = dict(dtype=torch.float32, device=device)
        out = {"mel": torch.empty((B, self.n_mels, M), **f32), "mel_len": torch.empty((B,), dtype=torch.int64, device=device),
               "pitch": torch.empty((B, M), **f32) if self.pitch else None,
               "energy": torch.empty((B, M), **f32) if self.energy else None}
        if self.tracker is not None:
            out["pyin"] = self.tracker.empty_outputs(B, S, device, pitch=out["pitch"])
        return out

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not audio.is_cuda or not audio_len.is_cuda:
            raise runtime.IspkError("AcousticFeatures needs GPU tensors; there is no CPU fallback")
        B, S = audio.shape
        if out is None:
            out = self.empty_outputs(B, S, audio.device)
        tables, fb_index = self.device_tables(audio.device)
        if self.tracker is None:
            runtime.audio_features(audio, audio_len, tables, fb_index, out["mel"], out["mel_len"], out.get("pitch"),
                                   out.get("energy"), self.tau_min, self.tau_max, float(self.sample_rate), self.threshold,
                                   self.pitch_mean, self.pitch_std)
            return out
        # pyin: the extractor's launch without its pitch, then the tracker's two, the contour straight into out["pitch"]
        runtime.audio_features(audio, audio_len, tables, fb_index, out["mel"], out["mel_len"], None, out.get("energy"))
        pitch = out.get("pitch")
        if pitch is None or not pitch.is_contiguous():
            raise ValueError("out['pitch']: a contiguous fp32 [B, M] tensor (take it from empty_outputs)")
        if out.get("pyin") is None or out["pyin"].get("pitch") is not pitch:
            out["pyin"] = self.tracker.empty_outputs(B, S, audio.device, pitch=pitch)
        self.tracker.normalised(self.pitch_mean, self.pitch_std)(audio, audio_len, out=out["pyin"])
        return out


def collate_audio(waveforms: Sequence[Tensor]) -> tuple[Tensor, Tensor]:
    """1-D fp32 waveforms -> (zero-padded fp32 [B, S_max], int64 lengths [B]), pinned when a GPU is present, ready for a
    non-blocking copy.  AcousticFeatures then gives M = the collator's padded width (the longest utterance's mel_len)."""
    lens = [int(w.shape[0]) for w in waveforms]
    for w in waveforms:
        if w.ndim != 1:
            raise ValueError(f"waveforms are 1-D, got {tuple(w.shape)}")
    pin = torch.cuda.is_available()
    audio = torch.zeros((len(waveforms), max(lens, default=0)), dtype=torch.float32, pin_memory=pin)
    for i, w in enumerate(waveforms):
        audio[i, :lens[i]] = w
    return audio, torch.tensor(lens, dtype=torch.int64).pin_memory() if pin else torch.tensor(lens, dtype=torch.int64)
