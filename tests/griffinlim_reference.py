"""Float64 reference of the Griffin-Lim mel inversion (isp_tts_amd/griffinlim.py, csrc/griffinlim.hip), written from the
definition: explicit zero padding, numpy.fft.rfft / irfft per frame, explicit overlap-add with the per-position envelope of the
utterance's own frames, a uint32 mirror of csrc/dropout.h's mix_seed / drop_hash, and the pseudo-inverse of the filterbank.
N = 1024, hop 256, K = 513 bins, w the periodic Hann window, 384 zeros on both sides, no centring (the feature extractor's
framing): T frames <-> n = 256 T samples."""
import numpy as np

N, HOP, K, PAD = 1024, 256, 513, 384
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def window() -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)


def pad(x: np.ndarray) -> np.ndarray:
    """xp[p] = x[p - 384] inside [0, n), 0 elsewhere; p < n + 768."""
    xp = np.zeros(x.shape[0] + 2 * PAD)
    xp[PAD:PAD + x.shape[0]] = x
    return xp


def stft(x: np.ndarray) -> np.ndarray:
    """x float64 [n] -> X complex128 [T, 513], T = (n + 768 - 1024) // 256 + 1 = n // 256 (the extractor's frame count)."""
    T = x.shape[0] // HOP
    xp, w = pad(np.asarray(x, dtype=np.float64)), window()
    return np.stack([np.fft.rfft(xp[HOP * f:HOP * f + N] * w) for f in range(T)]) if T else np.zeros((0, K), dtype=complex)


def istft(Y: np.ndarray) -> np.ndarray:
    """Y complex [T, 513] -> float64 [256 T]: windowed overlap-add of the frames over the envelope of their squared windows."""
    T = Y.shape[0]
    n, w = HOP * T, window()
    acc, env = np.zeros(n + 2 * PAD), np.zeros(n + 2 * PAD)
    for f in range(T):                                # ascending f
        Yf = Y[f].copy()
        Yf[0], Yf[-1] = Yf[0].real, Yf[-1].real        # irfft drops the imaginary parts of bins 0 and 512
        acc[HOP * f:HOP * f + N] += w * np.fft.irfft(Yf, N)
        env[HOP * f:HOP * f + N] += w * w
    assert T == 0 or env[PAD:PAD + n].min() > 0
    return acc[PAD:PAD + n] / env[PAD:PAD + n]


def project(X: np.ndarray, M: np.ndarray) -> np.ndarray:
    """Y = M X / |X|, M where |X| = 0."""
    mag = np.abs(X)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mag > 0, M * X / mag, M.astype(complex))


def step(x: np.ndarray, M: np.ndarray) -> np.ndarray:
    """One projection: x [256 T], M [T, 513] -> [256 T]."""
    assert x.shape[0] == HOP * M.shape[0]
    return istft(project(stft(x), M))


# ------------------------------------------------------------------------------------------------ csrc/dropout.h, in uint32
def mix_seed(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix32(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def drop_hash(seed: int, idx: np.ndarray) -> np.ndarray:
    """seed: the mixed 64-bit word; idx uint32."""
    return mix32(np.asarray(idx, dtype=np.uint32) ^ np.uint32(seed & M32)) ^ np.uint32(seed >> 32)


def hashed_phase(seed: int, T: int) -> np.ndarray:
    """u [T, 513] in [0, 1): (h >> 8) 2^-24 with h = drop_hash(mix_seed(seed), 513 f + k)."""
    idx = (np.arange(T, dtype=np.uint64)[:, None] * K + np.arange(K, dtype=np.uint64)[None, :]) & M32
    with np.errstate(over="ignore"):
        h = drop_hash(mix_seed(seed), idx.astype(np.uint32))
    return (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def initial(M: np.ndarray, seed: int) -> np.ndarray:
    """Synthesis alone of M exp(2 pi i u)."""
    return istft(M * np.exp(2j * np.pi * hashed_phase(seed, M.shape[0])))


def griffinlim(M: np.ndarray, n_iter: int, seed: int = 0, init=None, keep=()) -> np.ndarray:
    """n_iter projections from the hashed phase (or from `init`).  `keep`: iteration counts whose waveforms are returned as a
    dict {count: waveform} instead of the last waveform alone."""
    x = initial(M, seed) if init is None else np.asarray(init, dtype=np.float64)
    kept = {0: x} if 0 in keep else {}
    for i in range(1, n_iter + 1):
        x = step(x, M)
        if i in keep:
            kept[i] = x
    return kept if keep else x


def spectral_convergence(x: np.ndarray, M: np.ndarray) -> float:
    """|| |STFT(x)| - M ||_F / || M ||_F."""
    return float(np.linalg.norm(np.abs(stft(x)) - M) / np.linalg.norm(M))


# ------------------------------------------------------------------------------------------------------ mel <-> magnitude
def pinv(fb: np.ndarray) -> np.ndarray:
    """fb float64 [513, n_mels] (mel = fb^T magnitude) -> P [513, n_mels], the Moore-Penrose pseudo-inverse of fb^T."""
    return np.linalg.pinv(np.asarray(fb, dtype=np.float64).T)


def mel_to_linear(mel: np.ndarray, P: np.ndarray) -> np.ndarray:
    """log-mel [n_mels, T] -> M [T, 513] = max(P exp(mel), 0)."""
    return np.maximum(P @ np.exp(np.asarray(mel, dtype=np.float64)), 0.0).T


def log_mel(x: np.ndarray, fb: np.ndarray, clip: float = 1e-5) -> np.ndarray:
    """The extractor's log-mel of a waveform: log(max(fb^T |STFT(x)|, 1e-5)) [n_mels, T]."""
    return np.log(np.maximum((np.abs(stft(x)) @ np.asarray(fb, dtype=np.float64)).T, clip))
