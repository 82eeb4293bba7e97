"""The items, configurations and reference results that tests/test_screen_host.py and tests/test_gpu_screen.py share: made once
per process, never changed.  With T = runtime.SCREEN_TILE_SAMPLES the batch is 24 rows of S = 3 T + 8 samples, NaN behind every
item's length, so a read past a length shows.

The base of an item is keyed noise sign * U(0.05, 0.5): never zero, never near the rail.  Runs are painted over it: "+" / "-" set
+-0.9 (the item's peak, so at the rail under rail="max", and above the numeric rail 0.8), "0" sets zeros.  Every painted item
comes twice: as painted, and with every run turned into zeros in the same positions."""
import numpy as np

import screen_reference as R
from isp_tts_amd import runtime

RATE = 22050
T = runtime.SCREEN_TILE_SAMPLES
S = 3 * T + 8
RAIL_LEVEL = 0.9
BAND_DB = 60.0
BAND_FACTOR = 10.0 ** (-BAND_DB / 10.0)
MIN_BANDWIDTH_HZ = 7000.0
MIN_BAND_BIN = 326                                          # ceil(7000 * 1024 / 22050)
MAX_DC, MIN_PEAK = 0.01, 0.02
# name -> (rail, min_run); min_dropout_samples is set to min_run, so that the zero runs are judged at the same lengths
CONFIGS = {"max3": ("max", 3), "max5": ("max", 5), "num3": (0.8, 3), "num5": (0.8, 5)}
BAND_CUTS = (186, 372, 512)
FLOOR_DB = 90.0


def base(n, key):
    g = np.random.default_rng([31, key])
    return (g.choice([-1.0, 1.0], n) * g.uniform(0.05, 0.5, n)).astype(np.float32)


def paint(n, key, runs, zeros=False):
    x = base(n, key)
    for start, length, kind in runs:
        assert 0 <= start and start + length <= n
        x[start:start + length] = 0.0 if zeros or kind == "0" else (RAIL_LEVEL if kind == "+" else -RAIL_LEVEL)
    return x


def band_limited(n, cut, key):
    """White noise of n samples whose spectrum above cut / 1024 cycles per sample is scaled 90 dB down, peak 0.5."""
    g = np.random.default_rng([47, key])
    X = np.fft.rfft(g.standard_normal(n))
    f = np.arange(len(X)) / n                               # cycles per sample
    X[f > cut / 1024.0] *= 10.0 ** (-FLOOR_DB / 20.0)
    x = np.fft.irfft(X, n)
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


# the painted items: name -> (n, runs)
PAINTED = {
    # a run of each sign across a tile edge, and two of opposite sign that meet exactly at one
    "edges": (3 * T + 5, [(T - 2, 5, "+"), (2 * T - 4, 4, "+"), (2 * T, 6, "-"), (3 * T - 3, 5, "-")]),
    # a run that covers two whole tiles and more
    "cover": (3 * T + 5, [(T - 5, 2 * T + 7, "+"), (40, 7, "-")]),
    # a run from sample 0, one up to n - 1 (as zeros: padding, not dropouts) and one inside
    "ends": (2 * T, [(0, 6, "+"), (2 * T - 7, 7, "-"), (T + 100, 9, "+")]),
    # lengths min_run - 1 and min_run beside each other, for both values of min_run
    "beside": (T - 1, [(100, 2, "+"), (110, 3, "-"), (120, 4, "+"), (130, 5, "-"), (T - 3, 2, "+")]),
}
PLAIN_LENGTHS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1279, 1280)


def _items():
    items = {}
    for k, n in enumerate(PLAIN_LENGTHS):
        if 2 <= n <= 5:                                     # one run that is the whole item: counted from min_run on
            items[f"len{n}"] = np.full(n, RAIL_LEVEL, np.float32)
        elif n == 1279:                                     # the DC-offset item
            items["len1279_dc"] = (base(n, k) * np.float32(0.5) + np.float32(0.05)).astype(np.float32)
        else:
            items[f"len{n}"] = base(n if n else 16, k)      # (len0: samples behind a length of 0)
    for k, (name, (n, runs)) in enumerate(PAINTED.items()):
        items[name] = paint(n, 100 + k, runs)
        items[name + "_zero"] = paint(n, 100 + k, runs, zeros=True)
    # a numeric rail: one sample sets the peak, the plateaus lie below peak * rail_ratio and above 0.8
    x = base(T + 1, 200)
    x[17] = RAIL_LEVEL
    x[T - 4:T + 1], x[300:307] = 0.85, -0.85                # the first across the tile edge, up to n - 1
    items["plateau"] = x
    items["all_zero"] = np.zeros(2 * T + 100, np.float32)
    x = base(T, 201)
    x[5], x[T // 2], x[T // 2 + 1], x[T - 1] = np.nan, np.inf, -np.inf, np.nan
    x[1000:1004] = RAIL_LEVEL                               # NaN reads as 0: it ends this run and starts no other
    x[1004] = np.nan
    items["nonfinite"] = x
    for k, (cut, n) in enumerate(zip(BAND_CUTS, (4173, 6500, 9000))):
        items[f"band{cut}"] = band_limited(n, cut, k)
    return items


_CACHE = {}


def batch():
    """dict(names, clean [items], lens int64 [B], audio fp32 [B][S] with NaN behind each item)."""
    if "batch" not in _CACHE:
        items = _items()
        names = list(items)
        clean = [items[k] for k in names]
        lens = np.array([0 if k == "len0" else len(x) for k, x in zip(names, clean)], np.int64)
        audio = np.full((len(names), S), np.nan, np.float32)
        for b, (x, n) in enumerate(zip(clean, lens)):
            audio[b, :n] = x[:n]
        assert len(names) <= 24 and max(lens) <= S
        _CACHE["batch"] = dict(names=names, clean=clean, lens=lens, audio=audio)
    return _CACHE["batch"]


def long():
    """One item of 513 tiles and 5 samples: the per-item kernels stage the tile summaries 256 at a time and stride over the tiles'
    statistics 512 at a time, so both loops go round more than once; a rail run lies across the first staging edge, a zero run
    across the second."""
    if "long" not in _CACHE:
        n = 513 * T + 5
        x = paint(n, 300, [(256 * T - 3, 7, "+"), (512 * T - 2, 6, "0"), (300 * T + 9, 4, "-")])
        _CACHE["long"] = dict(names=["long"], clean=[x], lens=np.array([n], np.int64), audio=x[None, :])
    return _CACHE["long"]


def reference(config, which="batch"):
    """(the items' results, the batch's outputs) of batch() or long() under CONFIGS[config]."""
    if which == "long":
        if ("long", config) not in _CACHE:
            rail, min_run = CONFIGS[config]
            c = long()
            items = [R.screen_item(c["clean"][0], c["lens"][0], len(c["clean"][0]), rail=rail, min_run=min_run, min_dropout=min_run,
                                   band_factor=BAND_FACTOR, min_band_bin=MIN_BAND_BIN, max_dc=MAX_DC, min_peak=MIN_PEAK)]
            _CACHE[("long", config)] = (items, R.screen_batch(items))
        return _CACHE[("long", config)]
    if config not in _CACHE:
        rail, min_run = CONFIGS[config]
        c = batch()
        items = [R.screen_item(x, n, S, rail=rail, min_run=min_run, min_dropout=min_run, band_factor=BAND_FACTOR,
                               min_band_bin=MIN_BAND_BIN, max_dc=MAX_DC, min_peak=MIN_PEAK) for x, n in zip(c["clean"], c["lens"])]
        _CACHE[config] = (items, R.screen_batch(items))
    return _CACHE[config]


def torch_ltas(x):
    """float64 [513] from torch's own fp32 stft on the CPU (pocketfft), summed over the frames in float64: the yardstick for the
    kernel's fp32 transforms.  x fp32 with at least one frame."""
    import torch
    X = torch.stft(torch.from_numpy(np.asarray(x, np.float32)), R.FRAME, R.HOP, R.FRAME, torch.hann_window(R.FRAME), center=False,
                   return_complex=True)
    P = (X.real * X.real + X.imag * X.imag).double().numpy()            # fp32 [513, F]
    return P.sum(axis=1) / P.shape[1]
