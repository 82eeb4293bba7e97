"""float64 restatements for the audio front end's tests (no GPU, no package code): the sinc_interp_hann polyphase resampler
written as a direct sum from its definition, with the running-error bound of an fp32 evaluation, and the per-utterance
outlier filter and pooled statistics of the reference's compute_stats."""
import math

import numpy as np

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)


def dense_taps(orig, new, lpw=6, rolloff=0.99):
    """(k float64 [n, 2 width + o], o, n, width) by the definition: t = clamp((-p / n + (j - width) / o) base, -lpw, lpw),
    k = (t == 0 ? 1 : sin(pi t) / (pi t)) cos(pi t / (2 lpw))^2 base / o."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    k = np.empty((n, 2 * width + o), dtype=np.float64)
    for p in range(n):
        t = (-p / n + (np.arange(2 * width + o, dtype=np.float64) - width) / o) * base
        t = np.minimum(np.maximum(t, -lpw), lpw)
        s = np.ones_like(t)
        nz = t != 0
        s[nz] = np.sin(np.pi * t[nz]) / (np.pi * t[nz])
        k[p] = s * np.cos(np.pi * t / (2 * lpw)) ** 2 * (base / o)
    return k, o, n, width


def out_length(length, o, n):
    return -((-n * length) // o)


def _blocks(x, k, o, n, width):
    """x float64 [len] -> [ceil(len / o) n]: every output block of the zero-extended signal (width left, width + o right)."""
    J = k.shape[1]
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + o)])
    Q = -(-len(x) // o)
    idx = np.arange(Q)[:, None] * o + np.arange(J)[None, :]
    return (xp[idx] @ k.T).reshape(-1)


def resample64(x, k, o, n, width):
    """x [len] or [C, len] (any float dtype) -> (float64 [out_len], bound float64 [out_len]): the definition's direct sum on
    the channel mean, and sum_j |k[p, j]| mean_c |x_c[..]| (the running-error bound's magnitude term)."""
    x = np.asarray(x, dtype=np.float64)
    x = x[None] if x.ndim == 1 else x
    length = x.shape[1]
    ol = out_length(length, o, n)
    if length == 0:
        return np.zeros(0), np.zeros(0)
    y = _blocks(x.mean(0), k, o, n, width)[:ol]
    mag = _blocks(np.abs(x).mean(0), np.abs(k), o, n, width)[:ol]
    return y, mag


def taps_per_phase(k, lpw=6, o=None, n=None, width=None, rolloff=0.99):
    """The longest run of taps with |t| < lpw over the phases (the T of the bound)."""
    J = k.shape[1]
    base = min(o, n) * rolloff
    best = 0
    for p in range(n):
        t = (-p / n + (np.arange(J, dtype=np.float64) - width) / o) * base
        best = max(best, int((np.abs(t) < lpw).sum()))
    return best


# ------------------------------------------------------------------------------------------------------------- statistics
def bounds64(v):
    s = np.sort(np.asarray(v, dtype=np.float64))
    n = len(s)

    def quant(q):
        pos = q * (n - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, n - 1)
        return s[lo] + (pos - lo) * (s[hi] - s[lo])

    p25, p75 = quant(0.25), quant(0.75)
    return p25, p75, p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)


def kept64(v, positive_only):
    """The values of one utterance that the reference's compute_stats keeps, as float64 (empty for n = 0 or any NaN)."""
    v = np.asarray(v, dtype=np.float64)
    if len(v) == 0 or np.isnan(v).any():
        return np.zeros(0)
    _, _, lower, upper = bounds64(v)
    keep = (v > lower) & (v < upper)
    if positive_only:
        keep &= v > 0
    return v[keep]


def partial64(v, positive_only):
    """(count, mean, M2, min, max) of the kept values, two-pass float64."""
    x = kept64(v, positive_only)
    if len(x) == 0:
        return 0, 0.0, 0.0, np.inf, -np.inf
    mean = math.fsum(x) / len(x)
    return len(x), mean, math.fsum((x - mean) ** 2), x.min(), x.max()


def pooled64(rows, lens, positive_only):
    """(count, min, max, mean, std) over the kept values of all utterances, two-pass float64."""
    xs = [kept64(np.asarray(r)[:int(n)], positive_only) for r, n in zip(rows, lens)]
    x = np.concatenate(xs) if xs else np.zeros(0)
    if len(x) == 0:
        return 0, np.inf, -np.inf, float("nan"), float("nan")
    mean = math.fsum(x) / len(x)
    return len(x), x.min(), x.max(), mean, math.sqrt(math.fsum((x - mean) ** 2) / len(x))
