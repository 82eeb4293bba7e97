"""Float64 numpy restatement of the pitch tracker (ispk_pyin_observe_f32 / ispk_pyin_decode_f64, data.PitchTracker), written from
its definition (include/ispk.h) in librosa.pyin's own terms: difference function by direct sums, cumulative-mean normalisation,
troughs, the beta prior over 100 thresholds, the Boltzmann prior over the troughs below each, bins, then a dense Viterbi over
2 NB states with the block-maximum tie rule.  Nothing here is shared with the package: the tables are rebuilt from the formulas.

The observation also reports, per frame, how close the float64 computation comes to one of its decision points (`margins`), so that
a test can exclude the frames where a rounding of the device's fp32 transforms may legitimately flip a comparison."""
import math

import numpy as np

TINY = np.finfo(np.float64).tiny
HOP, WIN, FRAME = 256, 1024, 2048
N_THR = 100
LAMBDA = 2.0
NO_TROUGH = 0.01


def frames_of(n):
    return (n - HOP) // HOP + 1 if n >= HOP else 0


def beta_cdf_2_18(x):
    """I_x(2, 18) = 1 - (1 - x)^19 - 19 x (1 - x)^18, as the binomial sum over j >= 2 of C(19, j) x^j (1 - x)^(19 - j)."""
    x = np.asarray(x, dtype=np.float64)
    return sum(math.comb(19, j) * x ** j * (1.0 - x) ** (19 - j) for j in range(2, 20))


def thresholds_and_prior():
    grid = np.linspace(0.0, 1.0, N_THR + 1)
    return grid[1:], np.diff(beta_cdf_2_18(grid))


def n_bins(f_min, f_max, bps=10):
    return int(math.floor(12 * bps * math.log2(f_max / f_min))) + 1


def width_of(sr, bps=10, rate=35.92):
    return int(round(rate * 12 * HOP / sr)) * bps + 1


def periods(sr, f_min, f_max):
    return int(math.floor(sr / f_max)), min(int(math.ceil(sr / f_min)), 1022)


def frame(x, t):
    """Frame t of the item x: 2,048 samples from 256 t + 128 - 512, zeros outside the item."""
    x = np.asarray(x, dtype=np.float64)
    start = HOP * t + HOP // 2 - 512
    idx = np.arange(start, start + FRAME)
    inside = (idx >= 0) & (idx < len(x))
    out = np.zeros(FRAME)
    out[inside] = x[idx[inside]]
    return out


def difference(fr, max_period, dtype=np.float64):
    """d(tau), tau <= max_period, by direct sums of squares (float64), or - dtype=np.float32 - from energies and a cross-correlation
    carried out in fp32, the precision of the device's transforms."""
    if dtype == np.float64:
        win = np.lib.stride_tricks.sliding_window_view(fr, WIN)[:max_period + 1]
        return ((fr[None, :WIN] - win) ** 2).sum(axis=1)
    f = fr.astype(np.float32)
    head = np.zeros(FRAME, np.float32)
    head[:WIN] = f[:WIN]
    corr = np.fft.irfft(np.conj(np.fft.rfft(head)).astype(np.complex64) * np.fft.rfft(f).astype(np.complex64)).astype(np.float32)
    cs = np.concatenate([[0.0], np.cumsum(fr ** 2)])
    tau = np.arange(max_period + 1)
    return (cs[WIN] + (cs[tau + WIN] - cs[tau])) - 2.0 * corr[tau].astype(np.float64)


def observe_frame(fr, sr, f_min, nb, min_period, max_period, bps=10, dtype=np.float64):
    """(row float64 [NB], margins) of one frame.  margins: {"threshold": min |height - threshold| over troughs and thresholds,
    "neighbour": min |y[i] - y[i +- 1]| over the comparisons that decide a trough, "bin": [(distance of the pre-rounding bin value
    from the nearest half-integer, curvature a, lag)] per trough}."""
    thr, prior = thresholds_and_prior()
    d = difference(fr, max_period, dtype)
    tau = np.arange(1, max_period + 1)
    cmean = np.cumsum(d[1:]) / tau
    y = d[min_period:] / (cmean[min_period - 1:] + TINY)
    n = len(y)
    trough = np.zeros(n, bool)
    trough[1:-1] = (y[1:-1] < y[:-2]) & (y[1:-1] <= y[2:])
    trough[0] = y[0] < y[1]
    margins = {"threshold": np.inf, "neighbour": float(np.min(np.abs(np.diff(y)))) if n > 1 else np.inf, "bin": []}
    row = np.zeros(nb)
    idx = np.nonzero(trough)[0]
    if len(idx) == 0:
        return row, margins
    shift = np.zeros(n)
    a = y[2:] + y[:-2] - 2.0 * y[1:-1]
    b = (y[2:] - y[:-2]) / 2.0
    ok = np.abs(b) < np.abs(a)
    shift[1:-1][ok] = -b[ok] / a[ok]
    heights = y[idx]
    margins["threshold"] = float(np.min(np.abs(heights[:, None] - thr[None, :])))
    below = heights[:, None] < thr[None, :]                       # [troughs, thresholds]
    rank = np.cumsum(below, axis=0) - 1
    count = below.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        pmf = (1.0 - math.exp(-LAMBDA)) * np.exp(-LAMBDA * rank) / (1.0 - np.exp(-LAMBDA * count))[None, :]
    pmf[~below] = 0.0
    probs = pmf @ prior
    lowest = int(np.argmin(heights))
    probs[lowest] += NO_TROUGH * prior[:int((~below[lowest]).sum())].sum()
    f0 = sr / (min_period + idx + shift[idx])
    value = 12 * bps * np.log2(f0 / f_min)
    bins = np.clip(np.round(value), 0, nb - 1).astype(int)
    for j in range(len(idx)):                                     # lag order: the last candidate of a bin stands
        row[bins[j]] = probs[j]
        i = idx[j]
        curv = a[i - 1] if 0 < i < n - 1 else np.inf
        dist = abs(value[j] - math.floor(value[j]) - 0.5) if -1.0 < value[j] < nb else np.inf      # (clipped either way beyond)
        margins["bin"].append((dist, curv, min_period + i + shift[i]))
    return row, margins


def observe_item(x, sr, f_min=55.0, f_max=880.0, bps=10, dtype=np.float64):
    """(rows float64 [frames, NB], [margins per frame]) of one item."""
    nb = n_bins(f_min, f_max, bps)
    lo, hi = periods(sr, f_min, f_max)
    rows, margins = [], []
    for t in range(frames_of(len(x))):
        r, m = observe_frame(frame(x, t), sr, f_min, nb, lo, hi, bps, dtype)
        rows.append(r)
        margins.append(m)
    return (np.stack(rows) if rows else np.zeros((0, nb))), margins


def transition_tables(nb, width, switch=0.01):
    """(logtri [width], lognorm [NB], log stay, log switch, log init), every log as log(p + tiny)."""
    h = (width - 1) // 2
    tri = np.array([1.0 - abs(k - h) / (h + 1) for k in range(width)])
    norm = np.array([sum(tri[k] for k in range(width) if 0 <= i + k - h < nb) for i in range(nb)])
    return np.log(tri + TINY), np.log(norm + TINY), math.log(1.0 - switch + TINY), math.log(switch + TINY), math.log(1.0 / (2 * nb) + TINY)


def transition_matrix(nb, width, switch=0.01):
    """The dense 2 NB x 2 NB transition matrix the tables stand for (rows: source states)."""
    h = (width - 1) // 2
    tri = np.array([1.0 - abs(k - h) / (h + 1) for k in range(width)])
    local = np.zeros((nb, nb))
    for i in range(nb):
        for k in range(width):
            if 0 <= i + k - h < nb:
                local[i, i + k - h] = tri[k]
    local /= local.sum(axis=1, keepdims=True)
    return np.kron(np.array([[1.0 - switch, switch], [switch, 1.0 - switch]]), local)


def log_observations(rows):
    """float64 [frames, 2 NB] from voiced probabilities [frames, NB] (float64 sums of the values as given)."""
    rows = np.asarray(rows, dtype=np.float64)
    nb = rows.shape[1]
    vp = np.clip(rows.sum(axis=1), 0.0, 1.0)
    un = np.repeat(((1.0 - vp) / nb)[:, None], nb, axis=1)
    return np.log(np.concatenate([np.maximum(rows, 0.0), un], axis=1) + TINY), vp


def viterbi(logobs, tables, width):
    """(states int [frames], log_prob) over logobs float64 [frames, 2 NB].  Per target bin and source block (voiced, unvoiced) the
    maximum of delta'[i] + logtri over the source bins in ascending order, first maximum; then the voiced source on a tie; the
    lowest-index maximum ends the path.  Every operation is one float64 addition or comparison, in the order the header states."""
    logtri, lognorm, lstay, lswitch, linit = tables
    n, two = logobs.shape
    nb, h = two // 2, (width - 1) // 2
    if n == 0:
        return np.zeros(0, int), 0.0
    delta = linit + logobs[0]
    back = np.zeros((n, two), int)
    for t in range(1, n):
        dp = delta - np.concatenate([lognorm, lognorm])
        best = np.full((2, nb), -np.inf)
        arg = np.zeros((2, nb), int)
        for blk in range(2):
            pad = np.full(nb + 2 * h, -np.inf)
            pad[h:h + nb] = dp[blk * nb:(blk + 1) * nb]
            for k in range(width):                                # source bin c - h + k, ascending
                v = pad[k:k + nb] + logtri[width - 1 - k]
                better = v > best[blk]
                best[blk][better] = v[better]
                arg[blk][better] = (np.arange(nb) - h + k)[better]
            arg[blk] = np.where(np.isneginf(best[blk]), np.arange(nb), arg[blk])
        new = np.empty(two)
        for tgt in range(2):
            cv = best[0] + (lstay if tgt == 0 else lswitch)
            cu = best[1] + (lswitch if tgt == 0 else lstay)
            take_u = cu > cv
            new[tgt * nb:(tgt + 1) * nb] = np.where(take_u, cu, cv) + logobs[t, tgt * nb:(tgt + 1) * nb]
            back[t, tgt * nb:(tgt + 1) * nb] = np.where(take_u, nb + arg[1], arg[0])
        delta = new
    s = int(np.argmax(delta))
    logp = float(delta[s])
    states = np.zeros(n, int)
    for t in range(n - 1, 0, -1):
        states[t] = s
        s = back[t, s]
    states[0] = s
    return states, logp


def path_log_prob(states, logobs, tables, width):
    """The log-probability of a given path under the same model, in float64 (-inf for a step outside the band)."""
    logtri, lognorm, lstay, lswitch, linit = tables
    nb, h = logobs.shape[1] // 2, (width - 1) // 2
    if len(states) == 0:
        return 0.0
    total = linit + logobs[0, states[0]]
    for t in range(1, len(states)):
        i, j = states[t - 1], states[t]
        k = (j % nb) - (i % nb)
        if abs(k) > h:
            return -np.inf
        total = (total - lognorm[i % nb]) + logtri[h + k] + (lstay if (i < nb) == (j < nb) else lswitch) + logobs[t, j]
    return float(total)


def f0_of(states, f_min, nb, bps=10):
    states = np.asarray(states)
    return np.where(states < nb, f_min * 2.0 ** (states % nb / (12.0 * bps)), 0.0)


def track(x, sr, f_min=55.0, f_max=880.0, bps=10, switch=0.01):
    """The whole reference: (f0 Hz [frames], voiced bool [frames], states, log_prob, rows) of one item."""
    rows, _ = observe_item(x, sr, f_min, f_max, bps)
    nb, width = n_bins(f_min, f_max, bps), width_of(sr, bps)
    logobs, _ = log_observations(rows)
    states, logp = viterbi(logobs, transition_tables(nb, width, switch), width)
    return f0_of(states, f_min, nb, bps), states < nb, states, logp, rows


def clip(sr=22050, samples=20000, seed=0):
    """The test clip: seven harmonics of a 140 Hz tone gliding +-0.3 octave at 1.3 Hz with 5.5 Hz vibrato, silence at both ends, a
    noise burst in the middle, a 1e-3 noise floor.  float32 [samples]."""
    g = np.random.default_rng(seed)
    t = np.arange(samples) / sr
    f = 140.0 * 2.0 ** (0.3 * np.sin(2 * np.pi * 1.3 * t) + 0.01 * np.sin(2 * np.pi * 5.5 * t))
    phase = 2 * np.pi * np.cumsum(f) / sr
    x = sum(np.sin(h * phase) / h for h in range(1, 8)) * 0.2
    x[:2048] = 0.0
    x[-2048:] = 0.0
    x[9500:10500] = 0.1 * g.standard_normal(1000)
    x += 1e-3 * g.standard_normal(samples)
    return x.astype(np.float32)
