"""The recordings, configurations and reference plans that tests/test_segmenter_host.py and tests/test_gpu_segmenter.py share:
made once per process, never changed.  Bursts are synth.make_clip("harmonic", n, 0.5, sample_rate=8000), pauses exact zeros or
1e-3-scaled noise from a keyed stream; padding behind an item's length is NaN, so a read past a length shows.

With H = 256: a burst that ends at hop a and a gap of g hops behind it give the inactive frames a .. a + g - 4 (a frame is four
hops), so g - 3 inactive frames, a cut M = 256 (a + g / 2), and for pad = 1 and g = 9: e = 256 (a + 4), s = 256 (a + 5)."""
import numpy as np

import segmenter_reference as R
from isp_tts_amd import synth

RATE = 8000
H = 256
TOP_DB = 40.0
FACTOR = 10.0 ** (-TOP_DB / 10.0)
BUDGET = dict(min_silence_frames=6, target_samples=32 * H, max_samples=80 * H, min_samples=8 * H)
CONFIGS = {"max": dict(ref="max", pad_frames=1), "wide": dict(ref="max", pad_frames=8), "const": dict(ref=0.05, pad_frames=1)}
K_SMALL, K_LONG = 8, 256

_CLIPS = {}


def burst(n):
    if n not in _CLIPS:
        _CLIPS[n] = synth.make_clip("harmonic", n, 0.5, sample_rate=RATE).numpy()
    return _CLIPS[n]


def build(parts, key):
    """parts: [("b" burst | "z" zeros | "n" noise, samples)]."""
    out = []
    for i, (kind, n) in enumerate(parts):
        if kind == "b":
            out.append(burst(n))
        elif kind == "z":
            out.append(np.zeros(n, np.float32))
        else:
            out.append((1e-3 * np.random.default_rng([20260, key, i]).standard_normal(n)).astype(np.float32))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def _b(h):
    return ("b", h * H)


def _z(h):
    return ("z", h * H)


def _n(h):
    return ("n", h * H)


# name -> (parts, length or None for the whole item; "S+1" is resolved below)
SMALL = {
    "len0": ([("b", 1024)], 0), "len1": ([("b", 1)], None), "len255": ([("b", 255)], None), "len256": ([("b", 256)], None),
    "len257": ([("b", 257)], None), "len1023": ([("b", 1023)], None), "len1024": ([("b", 1024)], None),
    "len1025": ([("b", 1025)], None),
    "negative": ([_b(16)], -1), "beyond": ([_b(16)], "S+1"),
    "silent": ([_z(32)], None), "noise_only": ([_n(32)], None), "no_pause": ([_b(30)], None),
    "gap_below": ([_b(10), _z(8), _b(10)], None),             # 5 inactive frames = min_silence_frames - 1
    "gap_exact": ([_b(10), _z(9), _b(10)], None),             # 6 (and with pad 8 both sides clamp to M)
    "gap_noise": ([_b(10), _n(12), _b(10)], None),
    "lead": ([_z(12), _b(20), _z(9), _b(10)], None),          # a pause touching the start
    "trail": ([_b(20), _n(9), _b(10), _z(12)], None),         # and one touching the end
    "over_no_pause": ([_b(100)], None),                       # flag 1
    "look_again": ([_b(20), _z(9), _b(92), _z(9), _b(10)], None),
    "at_target": ([_b(28), _z(9), _b(10)], None),             # e_0 = 32 H = target_samples
    "below_target": ([_b(27), _z(9), _b(10)], None),
    "at_max": ([_b(20), _z(9), _b(47), _z(9), _b(10)], None),     # e_1 = 80 H = max_samples
    "above_max": ([_b(20), _z(9), _b(48), _z(9), _b(10)], None),
    "short_tail": ([_b(40), _z(9), _b(2)], None),             # flag 2
    "many": ([_b(32), _z(9)] * 12 + [_b(5)], None),           # wanted = 13 > K
    "ragged": ([("b", 5000), ("z", 3000), ("b", 7001), ("n", 2777), ("b", 3333)], None),
}
NAMES = list(SMALL)
_CACHE = {}


def small():
    """dict(audio fp32 [B][S] (NaN behind each item), clean [items], lens int64 [B], S, hops [per item])."""
    if "small" not in _CACHE:
        clean = [build(parts, k) for k, (parts, _) in enumerate(SMALL.values())]
        S = max(len(x) for x in clean) + 77
        lens = np.array([len(x) if n is None else (S + 1 if n == "S+1" else n) for x, (_, n) in zip(clean, SMALL.values())], np.int64)
        audio = np.full((len(clean), S), np.nan, np.float32)
        for b, x in enumerate(clean):
            audio[b, :len(x)] = x
        hops = [R.hop_sums(x, R.kept_len(n, S)) for x, n in zip(clean, lens)]
        _CACHE["small"] = dict(audio=audio, clean=clean, lens=lens, S=S, hops=hops)
    return _CACHE["small"]


def long():
    """Two items: about 2.2 M samples (8,600 frames: every per-item pass strides more than once - the frame passes, the
    candidate pass with its chunks of 8,192 frames, the choice with its tiles of 128 candidates) with pauses of 9 .. 12 hops
    whose starts lie 20, 30 and 50 hops apart in turn (the piece behind a 20 is below target_samples: that pause is passed
    over), zeros and noise in turn, and `look_again` beside it."""
    if "long" not in _CACHE:
        hops = 8600
        x = burst(hops * H + 100).copy()
        a, i = 38, 0
        while a + 12 < hops - 4:
            g = 9 + i % 4
            x[a * H:(a + g) * H] = build([("n" if i % 2 else "z", g * H)], 1000 + i)
            a, i = a + (20, 30, 50)[i % 3], i + 1
        clean = [x, build(SMALL["look_again"][0], 0)]
        S = len(x) + 5
        lens = np.array([len(c) for c in clean], np.int64)
        audio = np.full((2, S), np.nan, np.float32)
        for b, c in enumerate(clean):
            audio[b, :len(c)] = c
        _CACHE["long"] = dict(audio=audio, clean=clean, lens=lens, S=S, hops=[R.hop_sums(c, len(c)) for c in clean])
    return _CACHE["long"]


def reference(batch, config):
    """(the items' plans, the batch plan) of small() / long() under CONFIGS[config]."""
    key = (batch, config)
    if key not in _CACHE:
        c = small() if batch == "small" else long()
        cfg = CONFIGS[config]
        items = [R.plan_item(x, n, c["S"], FACTOR, cfg["ref"], cfg["pad_frames"], BUDGET["min_silence_frames"], BUDGET["target_samples"],
                             BUDGET["max_samples"], BUDGET["min_samples"], h=h) for x, n, h in zip(c["clean"], c["lens"], c["hops"])]
        _CACHE[key] = (items, R.plan_batch(items, K_SMALL if batch == "small" else K_LONG))
    return _CACHE[key]
