"""Float64 numpy restatement of the noise reducer (ispk_noise_profile_f64 / ispk_noise_reduce_f32, data.NoiseReducer), written
from its definition (include/ispk.h) one item at a time and not from the kernels.  The trim frames come
from tests/segmenter_reference.py (exactly rounded hop sums), the STFT / ISTFT from tests/denoiser_reference.py (explicit
reflection, numpy.fft per frame, explicit overlap-add).  No package code is imported.  Also the test signals, and torch's own
fp32 stft / istft chain on the CPU as the yardstick for what fp32 transforms cost."""
import numpy as np

from denoiser_reference import HOP, K, MIN_SAMPLES, N, istft, stft
from segmenter_reference import frame_powers, hop_sums, kept_len, margin, threshold  # noqa: F401  (margin: the tests' condition)

NO_PROFILE, SHORT = 1, 2
RATE = 22050


# ------------------------------------------------------------------------------------------------------------ profile
def noise_mask(x, n, factor, ref, guard):
    """bool [F]: which STFT frames of x[0, n) are noise frames (F = 1 + n // 256; n >= 513)."""
    p = frame_powers(hop_sums(x, n))
    T = len(p)
    active = p > threshold(p, factor, ref)
    F = 1 + n // HOP
    mask = np.zeros(F, dtype=bool)
    for f in range(2, n // HOP - 2 + 1):
        t = f - 2
        mask[f] = not active[max(0, t - guard):min(T, t + guard + 1)].any()
    return mask


def profile_item(x, n, S, factor, ref, guard, min_noise_frames):
    """One item: dict(n, frames, noise_frames, flags, noise float64 [513], mask)."""
    n = kept_len(n, S)
    if n < MIN_SAMPLES:
        return dict(n=n, frames=0, noise_frames=0, flags=SHORT | (NO_PROFILE if 0 < min_noise_frames else 0),
                    noise=np.zeros(K), mask=np.zeros(0, dtype=bool))
    x = np.asarray(x[:n], dtype=np.float64)
    mask = noise_mask(x, n, factor, ref, guard)
    count = int(mask.sum())
    noise = np.zeros(K)
    if count >= min_noise_frames and count > 0:
        noise = (np.abs(stft(x)[mask]) ** 2).sum(axis=0) / count
    return dict(n=n, frames=1 + n // HOP, noise_frames=count, flags=NO_PROFILE if count < min_noise_frames else 0, noise=noise,
                mask=mask)


def profile_batch(audio, lengths, factor, ref, guard, min_noise_frames):
    """([item], dict of arrays as the kernel's outputs)."""
    S = audio.shape[1]
    items = [profile_item(audio[b], lengths[b], S, factor, ref, guard, min_noise_frames) for b in range(audio.shape[0])]
    out = dict(noise=np.stack([it["noise"] for it in items]),
               noise_frames=np.array([it["noise_frames"] for it in items], np.int32),
               frames=np.array([it["frames"] for it in items], np.int32), flags=np.array([it["flags"] for it in items], np.int32))
    return items, out


# ------------------------------------------------------------------------------------------------------------ reduce
def raw_gain(X, noise, over, g_min):
    """g = max(1 - over noise[k] / |X|^2, g_min) where |X|^2 > 0, else g_min; X [F, 513]."""
    m2 = np.abs(X) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(m2 > 0, np.maximum(1.0 - over * np.asarray(noise, dtype=np.float64)[None, :] / m2, g_min), g_min)
    return g


def smooth_2d(g, Tt, Fk):
    """G_f[k] = sum w_t w_k g_{f+d}[k+e] / sum w_t w_k over the cells that exist: the definition, cell by cell."""
    F, Kb = g.shape
    G = np.zeros_like(g)
    for f in range(F):
        d = np.arange(max(-Tt, -f), min(Tt, F - 1 - f) + 1)
        wt = (Tt + 1 - np.abs(d)).astype(np.float64)
        for k in range(Kb):
            e = np.arange(max(-Fk, -k), min(Fk, Kb - 1 - k) + 1)
            w = wt[:, None] * (Fk + 1 - np.abs(e)).astype(np.float64)[None, :]
            G[f, k] = (w * g[f + d[:, None], k + e[None, :]]).sum() / w.sum()
    return G


def _smooth_axis(g, R, axis):
    """The triangular mean over R cells on either side along `axis`, renormalised over the cells that exist."""
    g = np.moveaxis(g, axis, 0)
    L = g.shape[0]
    num, den = np.zeros_like(g), np.zeros(L)
    for d in range(-R, R + 1):
        lo, hi = max(0, -d), min(L, L - d)
        if hi <= lo:
            continue
        num[lo:hi] += (R + 1 - abs(d)) * g[lo + d:hi + d]
        den[lo:hi] += R + 1 - abs(d)
    return np.moveaxis(num / den.reshape((L,) + (1,) * (g.ndim - 1)), 0, axis)


def smooth_separable(g, Tt, Fk):
    """Bins first, then frames, each renormalised: the same function, since the cells that exist form a rectangle."""
    return _smooth_axis(_smooth_axis(g, Fk, 1), Tt, 0)


def reduce_item(x, noise, over, g_min, Tt, Fk):
    """One item x [n] -> float64 [n]; below 513 samples a copy."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] < MIN_SAMPLES:
        return x.copy()
    X = stft(x)
    return istft(X * smooth_separable(raw_gain(X, noise, over, g_min), Tt, Fk), x.shape[0])


def floor_share(x, noise, over, g_min):
    """The share of (frame, bin) cells whose raw gain sits at the floor."""
    X = stft(np.asarray(x, dtype=np.float64))
    return float((raw_gain(X, noise, over, g_min) <= g_min).mean())


def reduce_batch(audio, lengths, noise, over, g_min, Tt, Fk, index=None, flags=None):
    """audio [B, S], lengths [B] (outside [0, S]: 0), noise [P, 513] -> float64 [B, S], zero from each length on; an item is
    copied below 513 samples, with bit 1 or 2 in its flag, or with a row outside [0, P)."""
    audio = np.asarray(audio, dtype=np.float64)
    B, S = audio.shape
    out = np.zeros((B, S))
    for b in range(B):
        n = kept_len(lengths[b], S)
        row = b if index is None else int(index[b])
        if n < MIN_SAMPLES or not 0 <= row < len(noise) or (flags is not None and int(flags[b]) & (NO_PROFILE | SHORT)):
            out[b, :n] = audio[b, :n]
        else:
            out[b, :n] = reduce_item(audio[b, :n], noise[row], over, g_min, Tt, Fk)
    return out


# ------------------------------------------------------------------------------------------------------------ signals
def make_signal(n, seed, bursts=None, sigma=1e-3, f0=220.0, rate=RATE):
    """fp32-representable float64 [n]: tone bursts (amplitude 0.3, three harmonics, 64-sample raised-cosine edges) plus white
    noise of standard deviation sigma everywhere.  bursts: [(start, end)] in samples; None: bursts of 1,536 samples every 6,144
    from sample 1,024 on.  At sigma = 1e-3 a pause's frame power is about 1e-6 against a burst's 5.9e-2: 17 dB below the
    threshold at top_db = 40."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / rate
    tone = 0.3 * sum(a * np.sin(2.0 * np.pi * h * f0 * t + h) for h, a in ((1, 1.0), (2, 0.5), (3, 0.25)))
    if bursts is None:
        bursts = [(s, s + 1536) for s in range(1024, n, 6144)]
    env = np.zeros(n)
    for s, e in bursts:
        s, e = max(0, s), min(n, e)
        if e <= s:
            continue
        seg = np.ones(e - s)
        r = min(64, (e - s) // 2)
        ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(r) + 0.5) / r)
        seg[:r], seg[e - s - r:] = ramp, ramp[::-1]
        env[s:e] = np.maximum(env[s:e], seg)
    x = tone * env + sigma * g.standard_normal(n)
    return x.astype(np.float32).astype(np.float64)


def burst_mask(n, bursts, spread=N):
    """bool [n]: samples within `spread` of a burst (what a frame that touches a burst can reach)."""
    m = np.zeros(n, dtype=bool)
    for s, e in bursts:
        m[max(0, s - spread):min(n, e + spread)] = True
    return m


# ------------------------------------------------------------------------------------------------------------ torch, fp32
def _window32():
    import torch
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)
    return torch.from_numpy(w.astype(np.float32))


def torch_profile(x, mask):
    """float64 [513]: |X_f[k]|^2 of torch.stft in fp32 on the CPU, summed in float64 over the frames of `mask`, over their count."""
    import torch
    X = torch.stft(torch.from_numpy(np.asarray(x, dtype=np.float32)), N, HOP, N, _window32(), center=True, pad_mode="reflect",
                   return_complex=True).T                                  # [F, 513]
    p = (X.real * X.real + X.imag * X.imag).numpy().astype(np.float64)
    return p[mask].sum(axis=0) / max(int(mask.sum()), 1)


def torch_reduce(x, noise, over, g_min, Tt, Fk):
    """float64 [n]: torch.stft and torch.istft in fp32 on the CPU around the gain (made in float64 from the fp32 spectrum and
    rounded to fp32): what the transforms alone cost in fp32."""
    import torch
    n = len(x)
    X = torch.stft(torch.from_numpy(np.asarray(x, dtype=np.float32)), N, HOP, N, _window32(), center=True, pad_mode="reflect",
                   return_complex=True)                                    # [513, F]
    G = smooth_separable(raw_gain(X.numpy().T.astype(np.complex128), noise, over, g_min), Tt, Fk)
    Y = X * torch.from_numpy(G.T.astype(np.float32))
    return torch.istft(Y, N, HOP, N, _window32(), center=True, length=n).numpy().astype(np.float64)
