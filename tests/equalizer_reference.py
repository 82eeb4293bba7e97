"""The equalizer's definition restated in float64 numpy, for the tests: the serial recurrence of include/ispk.h, the band designs
and the frequency response.  Nothing here imports the package.

The designs are made another way than data.equalize makes them: as the bilinear transform s = (1 - z^-1) / (K (1 + z^-1)),
K = tan(w0 / 2), of the RBJ cookbook's analogue prototypes (the cookbook's closed forms are that transform written out)."""
import math

import numpy as np

SEG = 8192


def _blt(num, den, K):
    """(b0, b1, b2, a1, a2) of (B0 s^2 + B1 s + B2) / (A0 s^2 + A1 s + A2) under the bilinear transform, a0 = 1."""
    def z(c):
        return np.array([c[0] + c[1] * K + c[2] * K * K, 2.0 * (c[2] * K * K - c[0]), c[0] - c[1] * K + c[2] * K * K])
    b, a = z(num), z(den)
    return np.array([b[0], b[1], b[2], a[1], a[2]]) / a[0]


def design(kind, rate, freq=0.0, gain_db=0.0, q=math.sqrt(0.5), coef=0.97):
    if kind == "preemphasis":
        return np.array([1.0, -coef, 0.0, 0.0, 0.0])
    if kind == "deemphasis":
        return np.array([1.0, 0.0, 0.0, -coef, 0.0])
    K = math.tan(math.pi * freq / rate)
    A = 10.0 ** (gain_db / 40.0)
    r = math.sqrt(A) / q
    num, den = {
        "lowpass": ([0.0, 0.0, 1.0], [1.0, 1.0 / q, 1.0]),
        "highpass": ([1.0, 0.0, 0.0], [1.0, 1.0 / q, 1.0]),
        "bandpass": ([0.0, 1.0 / q, 0.0], [1.0, 1.0 / q, 1.0]),
        "notch": ([1.0, 0.0, 1.0], [1.0, 1.0 / q, 1.0]),
        "peaking": ([1.0, A / q, 1.0], [1.0, 1.0 / (A * q), 1.0]),
        "lowshelf": ([A, A * r, A * A], [A, r, 1.0]),
        "highshelf": ([A * A, A * r, A], [1.0, r, A]),
    }[kind]
    return _blt(num, den, K)


def response(sos, freqs, rate):
    """complex128 H(e^(j w)) of the cascade, w = 2 pi f / rate, each section as a ratio of polynomials in z^-1."""
    w = 2.0 * np.pi * np.asarray(freqs, dtype=np.float64) / rate
    z1, z2 = np.exp(-1j * w), np.exp(-2j * w)
    h = np.ones_like(z1)
    for b0, b1, b2, a1, a2 in np.atleast_2d(sos):
        h = h * (b0 + b1 * z1 + b2 * z2) / (1.0 + a1 * z1 + a2 * z2)
    return h


def section(x, c, s0=None, s1=None):
    """One section over x float64 [R, n] (every row at once, serial over the samples), transposed direct form II from the
    states s0, s1 [R] (None: zero) -> (y [R, n], s0, s1)."""
    b0, b1, b2, a1, a2 = (float(v) for v in c)
    xt = np.ascontiguousarray(np.asarray(x, dtype=np.float64).T)
    R = xt.shape[1]
    s0 = np.zeros(R) if s0 is None else np.array(s0, dtype=np.float64)
    s1 = np.zeros(R) if s1 is None else np.array(s1, dtype=np.float64)
    yt = np.empty_like(xt)
    for i in range(xt.shape[0]):
        xi = xt[i]
        yi = b0 * xi + s0
        s0 = -a1 * yi + (b1 * xi + s1)
        s1 = -a2 * yi + b2 * xi
        yt[i] = yi
    return np.ascontiguousarray(yt.T), s0, s1


def cascade(x, sos, state=None):
    """The sections in order over x [R, n] from the joint state [R, 2 N] (None: zero) -> (y [R, n], every section's output
    [N, R, n], the joint state behind the last sample [R, 2 N])."""
    sos = np.atleast_2d(np.asarray(sos, dtype=np.float64))
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    outs, final = [], []
    for k, c in enumerate(sos):
        x, s0, s1 = section(x, c, None if state is None else state[:, 2 * k], None if state is None else state[:, 2 * k + 1])
        outs.append(x)
        final += [s0, s1]
    return x, np.stack(outs), np.stack(final, axis=1)


def kept(lens, S):
    lens = np.asarray(lens, dtype=np.int64)
    return np.where((lens < 0) | (lens > S), 0, lens)


def equalize_ref(audio, lens, sos):
    """audio [B, S] (any dtype; what lies at or past a length is not used), lens [B] -> (out float64 [B, S] with zeros from each
    length on, out_len int64 [B], P float64 [B]: the largest magnitude among the item's input and every section's output)."""
    audio = np.asarray(audio)
    B, S = audio.shape
    n = kept(lens, S)
    live = np.arange(S)[None, :] < n[:, None]
    x = np.where(live, audio, 0.0).astype(np.float64)
    y, outs, _ = cascade(x, sos)
    P = np.maximum(np.abs(x).max(axis=1, initial=0.0), np.where(live[None], np.abs(outs), 0.0).max(axis=(0, 2), initial=0.0))
    return np.where(live, y, 0.0), n, P


def reset_at_borders(x, sos):
    """A BROKEN equalizer: every 8,192-sample segment starts from zero state."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return np.concatenate([cascade(x[:, i:i + SEG], sos)[0] for i in range(0, x.shape[1], SEG)], axis=1)


def one_segment_memory(x, sos):
    """A BROKEN equalizer: a segment knows the segment before it and nothing older."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    parts = []
    for i in range(0, x.shape[1], SEG):
        lo = max(i - SEG, 0)
        parts.append(cascade(x[:, lo:i + SEG], sos)[0][:, i - lo:])
    return np.concatenate(parts, axis=1)
