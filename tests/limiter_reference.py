"""numpy restatement of the true-peak look-ahead limiter (ispk_limit_f32), written from its definition (include/ispk.h, DESIGN.md
section 4.27) in float64, one item at a time.  No package code is imported here.

    taps()                                 float64 [4, 12]: h[p][k], column k + 5
    limit_item(x, g, c, L)                 dict(out, e, r, m, s, true_peak, reduction) of one item x[0, n)
    limit_ref(audio, lens, gain, bounds, c, L)   the batch form: (out [B, S], out_len [B], true_peak [B], reduction [B])
    signals(n, c)                          the three test signals
"""
import numpy as np

TAPS, REACH_LO, REACH_HI = 12, 5, 6


def taps():
    t = np.arange(-REACH_LO, REACH_HI + 1, dtype=np.float64)[None, :] - np.arange(4, dtype=np.float64)[:, None] / 4.0
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    h = np.where(np.abs(t) < 6.0, sinc * np.cos(np.pi * t / 12.0) ** 2, 0.0)
    h[0] = np.where(t[0] == 0.0, 1.0, 0.0)           # sin(pi k) is an ulp of pi away from zero: the identity, exactly
    return h


def weights(L):
    k = np.arange(-L, L + 1, dtype=np.float64)
    w = np.cos(np.pi * k / (2.0 * (L + 1))) ** 2
    return w / w.sum()


def envelope(gx, h=None):
    """e[i] = max_p |sum_k h[p][k] gx[i + k]| over the item's n samples, zeros outside."""
    h = taps() if h is None else np.asarray(h, np.float64)
    n = gx.shape[0]
    pad = np.concatenate([np.zeros(REACH_LO), gx, np.zeros(REACH_HI)])
    e = np.zeros(n)
    for p in range(4):
        y = np.zeros(n)
        for j in range(TAPS):                         # k = j - 5, ascending
            y += h[p, j] * pad[j:j + n]
        e = np.maximum(e, np.abs(y))
    return e


def held_minimum(r, L):
    """m[j] = min over |k| <= L of r[j + k] for j in [-L, n + L), r = 1 outside [0, n): index j + L."""
    n = r.shape[0]
    pad = np.concatenate([np.ones(2 * L), r, np.ones(2 * L)])      # r over [-2 L, n + 2 L)
    m = np.full(n + 2 * L, np.inf)
    for k in range(2 * L + 1):
        m = np.minimum(m, pad[k:k + n + 2 * L])
    return m


def smooth(m, n, L, pad_with_ones=False):
    """s[i] = 1 - sum_k w[k] (1 - m[i + k]), m indexed from j = -L.  pad_with_ones: the WRONG variant that computes m on [0, n)
    only and pads it with ones - kept to show what the extended domain is for."""
    w = weights(L)
    d = 1.0 - m
    if pad_with_ones:
        d = d.copy()
        d[:L] = 0.0
        d[L + n:] = 0.0
    acc = np.zeros(n)
    for k in range(2 * L + 1):
        acc += w[k] * d[k:k + n]
    return 1.0 - acc


def limit_item(x, g, c, L, h=None, pad_with_ones=False):
    gx = np.float64(g) * np.asarray(x, np.float64)
    c = np.float64(c)
    n = gx.shape[0]
    if n == 0:
        z = np.zeros(0)
        return dict(out=z, e=z, r=z, m=np.ones(2 * L), s=z, true_peak=0.0, reduction=1.0)
    e = envelope(gx, h)
    with np.errstate(divide="ignore"):
        r = np.where(e > c, c / np.maximum(e, 1e-300), 1.0)
    m = held_minimum(r, L)
    s = smooth(m, n, L, pad_with_ones)
    out = np.clip(gx * s, -c, c)
    return dict(out=out, e=e, r=r, m=m, s=s, true_peak=float(e.max()), reduction=float(s.min()))


def kept_range(S, length, bound):
    """(lo, hi) of audio[b] that the entry point keeps."""
    n = S if length is None else int(length)
    if n < 0 or n > S:
        n = 0
    lo, hi = 0, n
    if bound is not None:
        lo, hi = int(bound[0]), int(bound[1])
        if not 0 <= lo <= hi <= S:
            lo = hi = 0
        hi = min(hi, n)
        lo = min(lo, hi)
    return lo, hi


def limit_ref(audio, lens, gain, bounds, c, L, h=None):
    audio = np.asarray(audio)
    B, S = audio.shape
    out, out_len = np.zeros((B, S)), np.zeros(B, np.int64)
    tp, red, s_all = np.zeros(B), np.ones(B), []
    for b in range(B):
        lo, hi = kept_range(S, None if lens is None else lens[b], None if bounds is None else bounds[b])
        it = limit_item(audio[b, lo:hi], 1.0 if gain is None else gain[b], c, L, h)
        out[b, :hi - lo] = it["out"]
        out_len[b], tp[b], red[b] = hi - lo, it["true_peak"], it["reduction"]
        s_all.append(it["s"])
    return out, out_len, tp, red, s_all


def signals(n, c, rate=22050.0, seed=5):
    """The three test signals: a Hann-enveloped 220 Hz sine at 1.5x full scale, white noise at 0.6 rms, a 3 kHz burst alternating
    0.2 / 1.8 every n / 8 samples."""
    t = np.arange(n, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * (t + 0.5) / n)
    sine = 1.5 * hann * np.sin(2.0 * np.pi * 220.0 * t / rate)
    noise = 0.6 * np.random.default_rng(seed).standard_normal(n)
    level = np.where((t // max(n // 8, 1)) % 2 == 0, 0.2, 1.8)
    burst = level * np.sin(2.0 * np.pi * 3000.0 * t / rate)
    return dict(sine=sine, noise=noise, burst=burst)


def true_peak_of(y, h=None):
    """The 4x true peak of a finished signal (the detector applied to the output)."""
    return float(envelope(np.asarray(y, np.float64), h).max()) if len(y) else 0.0
