"""Float64 restatement of audio conditioning (trim, ITU-R BS.1770-4 loudness, gain, PCM16) with numpy only: the definitions of
isp_tts_amd/csrc/condition.hip, evaluated sample by sample, one utterance at a time.  No package code is imported here."""
import math

import numpy as np

HOP, FRAME = 256, 1024
SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)     # f0 Hz, gain dB, Q
SHELF_VB_EXPONENT = 0.4996667741545416
HIGHPASS = (38.13547087602444, 0.5003270373238773)                     # f0 Hz, Q
BS1770_48K = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285),
              "shelf_a": (1.0, -1.69065929318241, 0.73248077421585),
              "highpass_b": (1.0, -2.0, 1.0),
              "highpass_a": (1.0, -1.99004745483398, 0.99007225036621)}


def k_weighting(fs):
    """((b, a) of the shelf, (b, a) of the high-pass), float64 [3] each, at sample rate fs."""
    f0, G, Q = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** SHELF_VB_EXPONENT
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, highpass


def biquad(b, a, x):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] from zero state (plain Python floats are float64)."""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    x1 = x2 = y1 = y2 = 0.0
    out = [0.0] * len(x)
    for n, xn in enumerate(x.tolist()):
        yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xn, y1, yn
        out[n] = yn
    return np.array(out, dtype=np.float64)


def frame_powers(x):
    """p_t, t < ceil(len / 256): the mean square of x[256 t, 256 t + 1024) over 1024 (the frame is cut at len)."""
    x = np.asarray(x, dtype=np.float64)
    n = -(-len(x) // HOP)
    return np.array([np.sum(x[HOP * t:HOP * t + FRAME] ** 2) / FRAME for t in range(n)], dtype=np.float64)


def trim_threshold(p, top_db, ref):
    return (p.max() if ref == "max" else float(ref)) * 10.0 ** (-top_db / 10.0)


def trim(x, top_db=60.0, pad_frames=0, ref="max"):
    """(start, end) of the utterance x (the valid samples only)."""
    n = len(x)
    if top_db is None:
        return 0, n
    p = frame_powers(x)
    if len(p) == 0:
        return 0, 0
    active = np.nonzero(p > trim_threshold(p, top_db, ref))[0]
    if len(active) == 0:
        return 0, 0
    f, l = int(active[0]), int(active[-1])
    return max(0, HOP * (f - pad_frames)), min(n, HOP * (l + pad_frames) + FRAME)


def block_powers(x, fs):
    """z_j of the K-weighted x (zero state at x[0]): blocks of 2 fs / 5 every fs / 10, wholly inside x."""
    if fs % 10:
        raise ValueError("fs / 10 is not a whole number of samples")
    (sb, sa), (hb, ha) = k_weighting(fs)
    y = biquad(hb, ha, biquad(sb, sa, np.asarray(x, dtype=np.float64)))
    step, block = fs // 10, 2 * fs // 5
    nblk = (len(y) - block) // step + 1 if len(y) >= block else 0
    return np.array([np.mean(y[j * step:j * step + block] ** 2) for j in range(nblk)], dtype=np.float64)


def gated(z):
    """(L, l_j, the relative threshold or None, mask of the absolute gate, mask of both)."""
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z) if len(z) else np.zeros(0)
    absolute = l > -70.0
    if not absolute.any():
        return -math.inf, l, None, absolute, absolute
    gamma = -0.691 + 10.0 * math.log10(np.mean(z[absolute])) - 10.0
    both = absolute & (l > gamma)
    if not both.any():
        return -math.inf, l, gamma, absolute, both
    return -0.691 + 10.0 * math.log10(np.mean(z[both])), l, gamma, absolute, both


def loudness(x, fs):
    return gated(block_powers(x, fs))[0]


def gain_for(L, peak, target_lufs=-23.0, peak_limit=10.0 ** (-1.0 / 20.0)):
    if target_lufs is None or L == -math.inf:
        return 1.0
    g = 10.0 ** ((target_lufs - L) / 20.0)
    if peak > 0:
        g = min(g, peak_limit / peak)
    return g


def condition(x, fs, target_lufs=-23.0, peak_limit=10.0 ** (-1.0 / 20.0), top_db=60.0, pad_frames=0, ref="max"):
    """One utterance (fp32 valid samples) -> dict(start, end, loudness, peak fp32, gain fp32, z, decisions ...)."""
    x = np.asarray(x, dtype=np.float32)
    start, end = trim(x, top_db, pad_frames, ref)
    seg = x[start:end]
    z = block_powers(seg, fs)
    L, l, gamma, absolute, both = gated(z)
    peak = np.float32(np.abs(seg).max()) if len(seg) else np.float32(0)
    g = gain_for(L, float(peak), target_lufs, peak_limit)
    return dict(start=start, end=end, loudness=L, peak=peak, gain=np.float32(g), z=z, l=l, gamma=gamma, absolute=absolute,
                both=both)


def margins_db(x, fs, top_db=60.0, ref="max"):
    """(smallest distance in dB of a block from either gate, of a frame from the trim threshold) for the utterance x: what
    must stay above the test's margin for gate and trim decisions to be comparable exactly across summation orders.  inf
    where there is nothing to decide."""
    x = np.asarray(x, dtype=np.float32)
    frame = math.inf
    if top_db is not None and len(x):
        p = frame_powers(x)
        thr = trim_threshold(p, top_db, ref)
        if thr > 0:
            with np.errstate(divide="ignore"):
                frame = float(np.abs(10.0 * np.log10(p / thr)).min())
        # thr == 0 (an all-zero item): p > 0 is false for every frame in any arithmetic
    start, end = trim(x, top_db, 0, ref)
    _, l, gamma, absolute, _ = gated(block_powers(x[start:end], fs))
    gate = math.inf
    if len(l):
        gate = float(np.abs(l + 70.0).min())
        if gamma is not None:
            gate = min(gate, float(np.abs(l[absolute] - gamma).min()))
    return gate, frame


# ------------------------------------------------------------------------------------------------------------------ PCM16
def _mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def _splitmix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9e3779b97f4a7c15) & m
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m
    return z ^ (z >> 31)


def dither(seed, b, n):
    """d[i] = (h(2 i) - h(2 i + 1)) 2^-32, i < n, for row b: h(k) = mix32(k ^ lo(r)) ^ hi(r), r = splitmix64(splitmix64(seed) + b)."""
    r = _splitmix64(_splitmix64(int(seed) & ((1 << 64) - 1)) + int(b))
    lo, hi = np.uint32(r & 0xffffffff), np.uint32(r >> 32)
    i = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h1 = _mix32((np.uint32(2) * i) ^ lo) ^ hi
        h2 = _mix32((np.uint32(2) * i + np.uint32(1)) ^ lo) ^ hi
    return (h1.astype(np.int64) - h2.astype(np.int64)).astype(np.float64) * 2.0 ** -32


def pcm16(x, length, use_dither=False, seed=0, b=0):
    """One row fp32 [S] -> int16 [S]: clamp(rint(32768 x + d)) (numpy's rint rounds half to even) below `length`, 0 past it."""
    x = np.asarray(x, dtype=np.float32)
    v = x.astype(np.float64) * 32768.0
    if use_dither:
        v = v + dither(seed, b, len(x))
    q = np.clip(np.rint(v), -32768.0, 32767.0)
    q[length:] = 0.0
    return q.astype(np.int16)
