"""The batches the declipper's tests share (tests/test_declip_host.py asserts on the CPU what makes the GPU comparisons in
tests/test_gpu_declip.py sound), each made once, with the reference's outputs per configuration.  Nothing here needs a GPU."""
import functools

import numpy as np

import declip_reference as D

RATE, S = 22050, 4096
LENS = (4096, 2900, 20)
GARBAGE = 7.5                                               # behind every length: at any rail, and finite
# name -> the Declipper's arguments (rail None: "max")
CONFIGS = {"default": dict(), "o1i1": dict(order=1, iterations=1), "o8": dict(order=8), "i1": dict(iterations=1),
           "mr1": dict(min_run=1), "mr64": dict(min_run=64), "rail": dict(rail=0.44)}
MIN_RUN = 3


def quiet_spot(y, start, length, level):
    """The first position >= start with |y| < level on [position - 2, position + length + 2)."""
    for p in range(max(start, 2), len(y) - length - 2):
        if np.abs(y[p - 2:p + length + 2]).max() < level:
            return p
    raise AssertionError("no quiet spot")


@functools.lru_cache(None)
def batch():
    """audio fp32 [3, S] with GARBAGE behind the lengths, lens, the clean signals, the rails and the planted runs {name: (item,
    start, length, sign)}."""
    audio = np.full((3, S), GARBAGE, np.float32)
    clean = np.zeros((3, S), np.float32)
    planted, rails = {}, []
    for b, n in enumerate(LENS):
        x = D.clip(RATE, S, seed=b)[1000:1000 + n] if n < 100 else D.clip(RATE, S, seed=b)[:n]
        y = D.hard_clip(x, 0.5) if n >= 100 else x.copy()                       # (the short item: the planted run alone)
        c = np.float32(np.abs(y).max())
        rails.append(c)

        def plant(name, start, length, sign):
            y[start:start + length] = sign * c
            planted[name] = (b, start, length, sign)
        if b == 0:
            plant("segment_edge", 509, 6, 1)                                    # across 512
            plant("window_edge", 766, 5, -1)                                    # across 768
            plant("at_zero", 0, 4, 1)
            plant("at_end", n - 4, 4, -1)
            plant("split", 1023, MIN_RUN, 1)                                    # 1 + (min_run - 1) across 1024
            q = quiet_spot(y, 1300, MIN_RUN - 1, 0.5 * c)
            plant("below_min_run", q, MIN_RUN - 1, 1)
            q = quiet_spot(y, q + 40, MIN_RUN, 0.5 * c)
            plant("min_run", q, MIN_RUN, -1)
            q = quiet_spot(y, 2000, 8, 0.5 * c)
            plant("plus", q, 4, 1)
            plant("minus", q + 4, 4, -1)                                        # a negative run at once behind a positive one
            q = quiet_spot(y, 2500, 64, 0.5 * c)
            plant("run64", q, 64, 1)
            q = quiet_spot(y, 3300, 63, 0.5 * c)
            plant("run63", q, 63, -1)
        elif b == 1:
            plant("at_end_ragged", n - 5, 5, 1)
            y[100], y[101] = np.float32("nan"), np.float32("inf")               # read as 0, copied through
        else:
            plant("short", 5, 4, 1)
        audio[b, :n], clean[b, :n] = y, x
    return dict(audio=audio, lens=np.array(LENS, np.int64), clean=clean, rails=rails, planted=planted)


@functools.lru_cache(None)
def reference(config="default", dtype="float64", skip=()):
    """(items, stacked) of the reference on the batch."""
    c = batch()
    kw = dict(CONFIGS[config])
    items = [D.declip_item(c["audio"][b], c["lens"][b], S, dtype=getattr(np, dtype), skip=b in skip, **kw) for b in range(3)]
    return items, D.declip_batch(items)


@functools.lru_cache(None)
def dense_limit():
    """Three items of 1,024 samples (two segments; windows [0, 768) and [256, 1024)) with single-sign runs planted on a quiet
    signal: 256 unknown samples inside [256, 768), so in both windows (both solved); the same with a 257th (both dense); the 256
    and three more in [10, 13), which only the first window holds (dense, the second solved)."""
    n = 1024
    base = (0.3 * D.clip(RATE, n, seed=3)).astype(np.float32)
    c = np.float32(0.9)
    audio = np.stack([base, base, base]).copy()
    for k in range(32):
        audio[:, 256 + 16 * k:256 + 16 * k + 8] = c
    audio[1, 256 + 16 * 31 + 8] = c
    audio[2, 10:13] = c
    lens = np.full(3, n, np.int64)
    items = [D.declip_item(audio[b], n, n) for b in range(3)]
    return dict(audio=audio, lens=lens, items=items, ref=D.declip_batch(items))


@functools.lru_cache(None)
def sinusoid():
    """A 300 Hz sinusoid clipped at 0.5: two thirds of every window are unknown."""
    x = (0.8 * np.sin(2 * np.pi * 300.0 * np.arange(S) / RATE)).astype(np.float32)
    return D.hard_clip(x, 0.5)
