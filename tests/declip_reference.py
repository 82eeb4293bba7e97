"""The declipper (include/ispk.h, csrc/declip.hip, data.Declipper) restated in numpy: Janssen's AR interpolation of the clipped
samples, window by window, in float64 - or, with dtype=np.longdouble, in the host's extended precision, which is what the tests
hold the float64 results against.  This is the specification the GPU tests compare against.  Nothing here knows about lanes."""
import numpy as np

from screen_reference import kept_len, runs_of

H, HALO, MAX_UNKNOWNS = 512, 256, 256
FLAGS = {"restored": 1, "dense": 2, "skipped": 4}


def clip(sr, n, seed=0):
    """A deterministic speech-like fp32 signal, peak 0.9: 120 Hz with vibrato, 29 harmonics (phases 0.05 h^2, so that the crest
    factor is a voice's and not a pulse train's), three formant resonators, a little noise and a slow envelope."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 120.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t + 0.3 * seed))
    phase = 2 * np.pi * np.cumsum(f0) / sr
    src = sum(np.cos(h * phase + 0.05 * h * h) / h for h in range(1, 30)) + 0.003 * rng.standard_normal(n)
    y = np.zeros(n)
    for freq, bw, gain in ((700.0, 130.0, 1.0), (1220.0, 70.0, 0.5), (2600.0, 160.0, 0.25)):
        r, th = np.exp(-np.pi * bw / sr), 2 * np.pi * freq / sr
        c1, c2 = 2 * r * np.cos(th), -r * r
        z = np.zeros(n)
        z1 = z2 = 0.0
        for i in range(n):
            z[i] = z0 = src[i] + c1 * z1 + c2 * z2
            z2, z1 = z1, z0
        y += gain * (1 - r) * z
    y *= 0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t + 1.0)
    return (0.9 * y / np.abs(y).max()).astype(np.float32)


def hard_clip(x, level):
    """x clipped at `level` times its own peak (fp32 in, fp32 out)."""
    c = np.float32(level * np.abs(x).max())
    return np.clip(x, -c, c).astype(np.float32)


def threshold(x, rail="max", rail_ratio=0.999):
    """(peak, thr) as the screen makes them: fp32, thr the fp32 product."""
    peak = np.float32(np.abs(x).max()) if len(x) else np.float32(0.0)
    return peak, (np.float32(peak * np.float32(rail_ratio)) if rail == "max" else np.float32(rail))


def unknown_mask(x, thr, min_run):
    """(mask, sign): the samples of the runs at the rail of at least min_run samples, and +1 / -1 there."""
    cls = np.where(x >= thr, 1, np.where(x <= -thr, 2, 0)) if thr > 0 else np.zeros(len(x), np.int64)
    mask, sign = np.zeros(len(x), bool), np.zeros(len(x))
    for s, m, c in runs_of(cls):
        if m >= min_run:
            mask[s:s + m] = True
            sign[s:s + m] = 1.0 if c == 1 else -1.0
    return mask, sign


def levinson(r, order):
    """a[0 .. order] with a[0] = 1, or None when a prediction error is not positive."""
    dt = r.dtype.type
    a = np.zeros(order + 1, r.dtype)
    a[0] = dt(1)
    e = r[0]
    for i in range(1, order + 1):
        acc = r[i] + np.dot(a[1:i], r[i - 1:0:-1])
        k = -acc / e
        a[1:i] = a[1:i] + k * a[i - 1:0:-1]
        a[i] = k
        e = e * (dt(1) - k * k)
        if not e > 0:
            return None
    return a


def solve_band(A, rhs, order):
    """x of A x = rhs for a symmetric positive definite A with half-bandwidth <= order: Cholesky and two triangular solves, or None
    when a pivot is not positive."""
    m = len(rhs)
    L = np.zeros_like(A)
    for j in range(m):
        lo, hi = max(0, j - order), min(m, j + order + 1)
        v = A[j:hi, j] - L[j:hi, lo:j] @ L[j, lo:j]
        if not v[0] > 0:
            return None
        L[j, j] = np.sqrt(v[0])
        L[j + 1:hi, j] = v[1:] / L[j, j]
    y = np.zeros_like(rhs)
    for i in range(m):
        lo = max(0, i - order)
        y[i] = (rhs[i] - L[i, lo:i] @ y[lo:i]) / L[i, i]
    x = np.zeros_like(rhs)
    for i in range(m - 1, -1, -1):
        hi = min(m, i + order + 1)
        x[i] = (y[i] - L[i + 1:hi, i] @ x[i + 1:hi]) / L[i, i]
    return x


def solve_window(w, unknown, sign, order, iterations, info=None):
    """The passes over one window: w (float64 or longdouble, the unknowns at their clipped values) -> the window with the unknowns
    restored, or None when an intermediate is not finite.  `info`: a dict that collects the largest condition number."""
    dt = w.dtype.type
    w = w.copy()
    N, U = len(w), np.flatnonzero(unknown)
    K = np.flatnonzero(~unknown)
    orig, s = w[U].copy(), sign[U].astype(w.dtype)
    for _ in range(iterations):
        r = np.array([np.dot(w[:N - k], w[k:]) if k < N else dt(0) for k in range(order + 1)], w.dtype)
        r[0] = r[0] * (dt(1) + dt(1e-9))
        if r[0] == 0:
            break
        a = levinson(r, order)
        if a is None:
            return None
        b = np.array([np.dot(a[:order + 1 - k], a[k:]) for k in range(order + 1)], w.dtype)
        dist = np.abs(U[:, None] - np.arange(N)[None, :])
        B = np.where(dist <= order, b[np.minimum(dist, order)], dt(0))           # [m, N]: the unknowns' rows of B
        rhs = -(B[:, K] @ w[K])
        A = B[:, U]
        if info is not None:
            info["cond"] = max(info.get("cond", 0.0), float(np.linalg.cond(A.astype(np.float64))))
        x = solve_band(A, rhs, order)
        if x is None or not np.isfinite(x.astype(np.float64)).all():
            return None
        w[U] = s * np.maximum(s * x, s * orig)
    return w


def declip_item(x, n, S, rail="max", rail_ratio=0.999, min_run=3, order=32, iterations=3, skip=False, dtype=np.float64, info=None):
    """One item: x fp32 (at least n samples are read when n is inside [0, S]) -> a dict of the outputs, `audio` fp32 [S], and the
    reference's own `mask` (the unknown samples), `kept` (those that were replaced) and `dense_segments`."""
    n = kept_len(n, S)
    raw = np.asarray(x[:n], np.float32)
    xf = np.where(np.isfinite(raw), raw, np.float32(0.0)).astype(np.float32)
    peak, thr = threshold(xf, rail, rail_ratio)
    out = np.zeros(S, np.float32)
    out[:n] = raw
    r = dict(n=n, thr=thr, clip_samples=0, restored=0, windows=0, dense=0, flags=FLAGS["skipped"] if skip else 0,
             mask=np.zeros(n, bool), kept=np.zeros(n, bool), dense_segments=[])
    if not skip:
        mask, sign = unknown_mask(xf, thr, min_run)
        r["mask"], r["clip_samples"] = mask, int(mask.sum())
        for j in range(-(-n // H)):
            s0, s1 = H * j, min(H * j + H, n)
            own = int(mask[s0:s1].sum())
            if own == 0:
                continue
            lo, hi = max(s0 - HALO, 0), min(s0 + H + HALO, n)
            w = None
            if mask[lo:hi].sum() <= MAX_UNKNOWNS:
                w = solve_window(xf[lo:hi].astype(dtype), mask[lo:hi], sign[lo:hi], order, iterations, info)
            if w is None:
                r["dense"] += 1
                r["dense_segments"].append(j)
                continue
            keep = np.flatnonzero(mask[s0:s1]) + s0
            out[keep] = w[keep - lo].astype(np.float32)
            r["kept"][keep] = True
            r["windows"] += 1
            r["restored"] += own
        r["flags"] |= (FLAGS["restored"] if r["restored"] else 0) | (FLAGS["dense"] if r["dense"] else 0)
    fin = np.where(np.isfinite(out[:n]), out[:n], np.float32(0.0))
    r["peak"] = np.float32(np.abs(fin).max()) if n else np.float32(0.0)
    r["audio"], r["audio_len"] = out, n
    return r


DTYPES = dict(audio_len=np.int64, thr=np.float32, peak=np.float32, clip_samples=np.int64, restored=np.int64, windows=np.int32,
              dense=np.int32, flags=np.int32)


def declip_batch(items):
    """The items' outputs stacked as the kernel lays them out."""
    r = {k: np.array([it[k] for it in items], dtype=dt) for k, dt in DTYPES.items()}
    r["audio"] = np.stack([it["audio"] for it in items])
    return r


def sdr_db(clean, got, where):
    """10 log10 of the clean energy over the error energy on the samples `where` (float64)."""
    c, g = clean[where].astype(np.float64), got[where].astype(np.float64)
    return 10.0 * np.log10(np.sum(c * c) / np.sum((c - g) ** 2))


def ulps(a, b):
    """The distance of two fp32 arrays in units in the last place (of finite values of one sign or zero)."""
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
