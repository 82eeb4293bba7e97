"""The screen (include/ispk.h, csrc/screen.hip, data.Screen) restated in numpy: float64 and Python integers, sums by math.fsum.
This is the specification the GPU tests compare against.  Nothing here knows about tiles."""
import math

import numpy as np
import torch

HOP, FRAME, BINS = 256, 1024, 513
FLAGS = {"clipped": 1, "narrow": 2, "dc": 4, "dropout": 8, "nonfinite": 16, "quiet": 32, "short": 64}
INT_KEYS = ("nonfinite", "clip_runs", "clip_samples", "clip_longest", "clip_first", "dropout_runs", "dropout_samples",
            "dropout_longest", "band_bin", "flags")
WINDOW = torch.hann_window(FRAME, dtype=torch.float32).numpy().astype(np.float64)      # the extractor's fp32 periodic Hann


def kept_len(n, S):
    return int(n) if 0 <= n <= S else 0


def runs_of(cls):
    """[(start, length, class)] of the maximal stretches of one non-zero class in an integer array."""
    cls = np.asarray(cls)
    if len(cls) == 0:
        return []
    edge = np.flatnonzero(np.diff(cls) != 0) + 1
    starts = np.concatenate([[0], edge])
    ends = np.concatenate([edge, [len(cls)]])
    return [(int(s), int(e - s), int(cls[s])) for s, e in zip(starts, ends) if cls[s] != 0]


def frames_of(n):
    return max(0, (n - FRAME) // HOP + 1)


def spectra(x):
    """float64 [F, 513]: |X_f[k]|^2 of the frames [256 f, 256 f + 1024) of x times the window, no padding."""
    F = frames_of(len(x))
    if F == 0:
        return np.zeros((0, BINS))
    idx = HOP * np.arange(F)[:, None] + np.arange(FRAME)[None, :]
    X = np.fft.rfft(x.astype(np.float64)[idx] * WINDOW, axis=1)
    return X.real ** 2 + X.imag ** 2


def band_of(ltas, F, band_factor):
    """(band_bin, top, level): the last bin at or above top * band_factor, top the largest of bins 2 .. 512."""
    top = float(ltas[2:].max()) if F else 0.0
    level = top * band_factor
    if F == 0 or top == 0.0:
        return -1, top, level
    return int(np.flatnonzero(ltas >= level).max()), top, level


def screen_item(x, n, S, rail="max", rail_ratio=0.999, min_run=3, min_dropout=110, band_factor=1e-6, min_band_bin=-1,
                max_dc=0.01, min_peak=0.0):
    """One item: x fp32 (at least n samples are read when n is inside [0, S]) -> a dict of the outputs, `ltas` float64 [513], and
    the reference's own `thr`, `F`, `level` (the band threshold) and the run lists `rail_runs`, `zero_runs`."""
    n = kept_len(n, S)
    raw = np.asarray(x[:n], np.float32)
    fin = np.isfinite(raw)
    x = np.where(fin, raw, np.float32(0.0)).astype(np.float32)
    r = {"nonfinite": int(n - fin.sum())}
    peak = np.float32(np.abs(x).max()) if n else np.float32(0.0)
    xd = x.astype(np.float64)
    r["peak"] = peak
    r["dc"] = math.fsum(xd) / n if n else 0.0
    r["power"] = math.fsum(xd * xd) / n if n else 0.0              # the squares of fp32 values are exact in float64
    r["mean_abs"] = math.fsum(np.abs(xd)) / n if n else 0.0

    thr = np.float32(peak * np.float32(rail_ratio)) if rail == "max" else np.float32(rail)
    cls = np.where(x >= thr, 1, np.where(x <= -thr, 2, 0)) if thr > 0 else np.zeros(n, np.int64)
    rail_runs = runs_of(cls)
    counted = [(s, m) for s, m, _ in rail_runs if m >= min_run]
    r["clip_runs"], r["clip_samples"] = len(counted), sum(m for _, m in counted)
    r["clip_longest"] = max([m for _, m, _ in rail_runs], default=0)
    r["clip_first"] = counted[0][0] if counted else -1

    zero_runs = runs_of((x == 0).astype(np.int64))
    drops = [(s, m) for s, m, _ in zero_runs if m >= min_dropout and s > 0 and s + m < n]
    r["dropout_runs"], r["dropout_samples"] = len(drops), sum(m for _, m in drops)
    r["dropout_longest"] = max([m for _, m in drops], default=0)

    F = frames_of(n)
    P = spectra(x)
    ltas = np.array([math.fsum(P[:, k]) / F for k in range(BINS)]) if F else np.zeros(BINS)
    r["ltas"] = ltas
    r["band_bin"], top, level = band_of(ltas, F, band_factor)

    f = 0
    f |= FLAGS["clipped"] if r["clip_runs"] > 0 else 0
    f |= FLAGS["narrow"] if min_band_bin >= 0 and 0 <= r["band_bin"] < min_band_bin else 0
    f |= FLAGS["dc"] if abs(r["dc"]) > max_dc else 0
    f |= FLAGS["dropout"] if r["dropout_runs"] > 0 else 0
    f |= FLAGS["nonfinite"] if r["nonfinite"] > 0 else 0
    f |= FLAGS["quiet"] if float(peak) <= min_peak else 0
    f |= FLAGS["short"] if F == 0 else 0
    r["flags"] = f
    r.update(thr=thr, F=F, n=n, top=top, level=level, rail_runs=rail_runs, zero_runs=zero_runs, frame_power=P)
    return r


DTYPES = dict(nonfinite=np.int32, peak=np.float32, dc=np.float64, power=np.float64, clip_runs=np.int32, clip_samples=np.int64,
              clip_longest=np.int64, clip_first=np.int64, dropout_runs=np.int32, dropout_samples=np.int64, dropout_longest=np.int64,
              ltas=np.float64, band_bin=np.int32, flags=np.int32)


def screen_batch(items):
    """The items' outputs stacked as the kernel lays them out."""
    return {k: np.array([it[k] for it in items], dtype=dt) for k, dt in DTYPES.items()}
