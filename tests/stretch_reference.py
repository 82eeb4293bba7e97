"""Float64 numpy restatement of the time stretch (ispk_stretch_f32, data.TimeStretch), written from its definition (include/ispk.h,
DESIGN.md section 4.33) in the textbook form - angles, the expected advance w_k and wrap() - one item at a time and not from the
kernels, which multiply unit phasors instead.  The STFT is tests/denoiser_reference.py's (explicit reflection, numpy.fft per
frame); the overlap-add is written out, so a `wanted` beyond torch.istft's default length needs no special case.  No package code
is imported.  Also the modulo-2-pi form, the mixed chain (torch's fp32 stft, float64 phases, fp32 inverse) whose error against
the reference is what the GPU tests' bound is made of, and the test signals."""
import numpy as np

from denoiser_reference import HOP, K, MIN_SAMPLES, N, stft, window

SHORT, TRUNCATED, BAD_RATE = 1, 2, 4
RATE_MIN, RATE_MAX = 0.5, 2.0
RATE_HZ = 22050
TWO_PI = 2.0 * np.pi


def kept_len(n, S):
    n = int(n)
    return n if 0 <= n <= S else 0


def plan(n, r):
    """(F, Fo, wanted) of an item of n >= 513 samples at rate r: F = 1 + n // 256 analysis frames, Fo = the smallest j >= 0 with
    j r >= F (float64 products), wanted = round-half-even(n / r) from the float64 quotient."""
    r = float(r)
    F = 1 + n // HOP
    j = 0
    while float(j) * r < F:
        j += 1
    return F, j, int(round(n / r))


def frame_times(Fo, r):
    """(i_j, a_j), j < Fo: t_j = j r as a float64 product, i_j = floor(t_j), a_j = t_j - i_j."""
    t = np.arange(Fo, dtype=np.float64) * float(r)
    i = np.floor(t).astype(np.int64)
    return i, t - i


def wrap(d):
    return d - TWO_PI * np.round(d / TWO_PI)


def vocoder_frames(X, r, Fo, form="textbook"):
    """X complex [F, 513] -> Y complex128 [Fo, 513].  Magnitudes interpolated between the frames i_j and i_j + 1 (X_F = X_{F+1} =
    0), phases accumulated: the textbook recurrence with w_k and wrap(), or (form="modulo") P_{j+1} = (P_j + arg X_{i_j+1} - arg
    X_{i_j}) mod 2 pi.  arg 0 = 0 (numpy.angle)."""
    X = np.asarray(X, dtype=np.complex128)
    Xp = np.concatenate([X, np.zeros((2, X.shape[1]), dtype=np.complex128)])
    i, a = frame_times(Fo, r)
    mag, ang = np.abs(Xp), np.angle(Xp)
    M = (1.0 - a)[:, None] * mag[i] + a[:, None] * mag[i + 1]
    P = np.zeros((Fo, X.shape[1]))
    P[0] = ang[0]
    if form == "textbook":
        w = np.pi * np.arange(X.shape[1], dtype=np.float64) / 2.0
        for j in range(Fo - 1):
            P[j + 1] = P[j] + w + wrap(ang[i[j] + 1] - ang[i[j]] - w)
    else:
        assert form == "modulo"
        for j in range(Fo - 1):
            P[j + 1] = np.mod(P[j] + ang[i[j] + 1] - ang[i[j]], TWO_PI)
    return M * np.exp(1j * P)


def overlap_add(frames, length, dtype=np.float64):
    """frames real [Fo, 1024] (the inverse transforms) -> [length]: the windowed overlap-add over the envelope of the squared
    windows of the frames j < Fo, both in ascending j, samples [0, length) behind the 512 samples of padding."""
    w = window().astype(dtype)
    Fo = frames.shape[0]
    total = max(HOP * (Fo - 1) + N, N // 2 + length)
    acc, env = np.zeros(total, dtype=dtype), np.zeros(total, dtype=dtype)
    for j in range(Fo):
        acc[HOP * j:HOP * j + N] += w * frames[j].astype(dtype)
        env[HOP * j:HOP * j + N] += w * w
    assert (env[N // 2:N // 2 + length] > 0).all(), "a sample below `length` lies under no output frame"
    return acc[N // 2:N // 2 + length] / env[N // 2:N // 2 + length]


def synthesize(Y, length):
    Y = Y.copy()
    Y[:, 0], Y[:, -1] = Y[:, 0].real, Y[:, -1].real                       # irfft drops the imaginary parts of bins 0 and 512
    return overlap_add(np.fft.irfft(Y, N, axis=1), length)


def stretch_item(x, r, form="textbook"):
    """One item x [n], n >= 513 -> float64 [wanted]."""
    x = np.asarray(x, dtype=np.float64)
    F, Fo, wanted = plan(x.shape[0], r)
    return synthesize(vocoder_frames(stft(x), r, Fo, form), wanted)


def bad_rate(r):
    return not (RATE_MIN <= float(r) <= RATE_MAX)                         # NaN compares false


def lengths(n, r, out_samples):
    """(out_len, wanted, flags) of an item."""
    flags = (SHORT if n < MIN_SAMPLES else 0) | (BAD_RATE if bad_rate(r) else 0)
    wanted = n if flags else plan(n, r)[2]
    if wanted > out_samples:
        flags |= TRUNCATED
    return min(wanted, out_samples), wanted, flags


def stretch_batch(audio, lens, rates, out_samples, cache=None):
    """audio [B, S], lens [B] (outside [0, S]: 0), rates a float or [B] -> (float64 [B, out_samples] with zeros from out_len on,
    out_len, wanted int64 [B], flags int32 [B]); a short item or one with a bad rate is copied."""
    audio = np.asarray(audio, dtype=np.float64)
    B, S = audio.shape
    out = np.zeros((B, out_samples))
    ol, wa, fl = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int32)
    for b in range(B):
        n = kept_len(lens[b], S)
        r = rates[b] if np.ndim(rates) else rates
        ol[b], wa[b], fl[b] = lengths(n, r, out_samples)
        y = audio[b, :n] if fl[b] & (SHORT | BAD_RATE) else stretch_item(audio[b, :n], r)
        out[b, :ol[b]] = y[:ol[b]]
    return out, ol, wa, fl


# ------------------------------------------------------------------------------------------------------------ torch, fp32
def mixed_item(x, r):
    """float64 [wanted]: torch.stft in fp32 on the CPU, the phase arithmetic in float64 reduced modulo 2 pi, the inverse transforms
    and the overlap-add in fp32 - what fp32 transforms around exact phases cost."""
    import torch
    x = np.asarray(x, dtype=np.float64)
    F, Fo, wanted = plan(x.shape[0], r)
    w32 = torch.from_numpy(window().astype(np.float32))
    X = torch.stft(torch.from_numpy(x.astype(np.float32)), N, HOP, N, w32, center=True, pad_mode="reflect", return_complex=True).T
    assert X.shape == (F, K) and X.dtype == torch.complex64
    Y = vocoder_frames(X.numpy().astype(np.complex128), r, Fo, "modulo").astype(np.complex64)
    Y[:, 0], Y[:, -1] = Y[:, 0].real, Y[:, -1].real
    y = torch.fft.irfft(torch.from_numpy(Y), N, dim=1)
    assert y.dtype == torch.float32
    return overlap_add(y.numpy(), wanted, np.float32).astype(np.float64)


def relative_error(got, want):
    """max |got - want| over the peak of `want`."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------ signals
def noise_signal(n, seed):
    """fp32-representable float64 [n]: white Gaussian noise of standard deviation 0.1."""
    x = 0.1 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32).astype(np.float64)


def glide_signal(n, seed, rate=RATE_HZ):
    """fp32-representable float64 [n]: a tone of 7 harmonics (amplitudes 0.2 / h) gliding from 150 to 300 Hz over the item, plus
    white noise of 0.05."""
    t = np.arange(n, dtype=np.float64)
    f0 = 150.0 + 150.0 * t / max(n, 1)
    ph = TWO_PI * np.cumsum(f0) / rate
    x = sum(0.2 / h * np.sin(h * ph) for h in range(1, 8)) + 0.05 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32).astype(np.float64)


def tone_signal(n, seed, hz=440.0, rate=RATE_HZ):
    """fp32-representable float64 [n]: a sinusoid of amplitude 0.3 with white noise 54 dB below it (the property tests': a pure
    tone is ill-conditioned, its empty bins hold rounding noise whose phase accumulates)."""
    x = 0.3 * np.sin(TWO_PI * hz * np.arange(n) / rate) + 0.3 * 10.0 ** (-54.0 / 20.0) * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32).astype(np.float64)


def signal(n, seed):
    """The numeric tests' inputs: noise for an even seed, the glide for an odd one."""
    return noise_signal(n, seed) if seed % 2 == 0 else glide_signal(n, seed)


def peak_bin(x, nfft=8192):
    """The bin of the largest magnitude of a Hann-windowed transform of the middle `nfft` samples of x."""
    x = np.asarray(x, dtype=np.float64)
    s = max(0, (len(x) - nfft) // 2)
    seg = x[s:s + nfft]
    return int(np.abs(np.fft.rfft(seg * np.hanning(len(seg)), nfft)).argmax())
