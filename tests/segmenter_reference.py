"""numpy restatement of the segmenter (ispk_segment_plan / ispk_segment_gather_f32), written from its definition (include/ispk.h,
DESIGN.md section 4.30) one item at a time and not from the kernels: frame powers, candidates, the choice loop verbatim, levels,
gather.  No package code is imported.  All integers; `//` floors.  The hop sums are exactly rounded (math.fsum of the squares,
which float64 holds exactly), so a kernel's distance to them is the kernel's own error."""
import math

import numpy as np

HOP, FRAME = 256, 1024
OVER, SHORT, CUT = 1, 2, 4


def kept_len(n, S):
    n = int(n)
    return n if 0 <= n <= S else 0


def hop_sums(x, n):
    """float64 [T]: the sum of squares of x[256 t, min(256 t + 256, n)), T = ceil(n / 256)."""
    sq = np.asarray(x[:n], dtype=np.float64) ** 2
    T = -(-n // HOP)
    return np.array([math.fsum(sq[HOP * t:HOP * t + HOP]) for t in range(T)], dtype=np.float64)


def frame_powers(h):
    """p_t = (((h_t + h_{t+1}) + h_{t+2}) + h_{t+3}) / 1024 with hops at or past T left out."""
    T = len(h)
    p = h.copy()
    for k in (1, 2, 3):
        p[:max(T - k, 0)] += h[k:]
    return p / float(FRAME)


def threshold(p, factor, ref):
    """ref: "max" or a constant."""
    if ref == "max":
        return (float(p.max()) if len(p) else 0.0) * factor
    return float(ref) * factor


def margin(x, n, factor, ref):
    """(min_t |p_t - thr| / thr, thr); (inf, thr) for thr == 0 or an item without a frame."""
    p = frame_powers(hop_sums(x, n))
    thr = threshold(p, factor, ref)
    if thr == 0.0 or len(p) == 0:
        return math.inf, thr
    return float(np.abs(p - thr).min() / thr), thr


def plan_item(x, n, S, factor, ref, pad, min_silence_frames, target_samples, max_samples, min_samples, h=None):
    """One item: dict(first, last, p, active, candidates [(e, s)], segments [(s, e)] (every emit), flags, visits (how often each
    boundary index 0 .. n was looked at), levels [(frames, speech_frames, speech_power, noise_power)]).  h: hop_sums(x, kept
    length), where a caller has them already."""
    n = kept_len(n, S)
    p = frame_powers(hop_sums(x, n) if h is None else h)
    T = len(p)
    thr = threshold(p, factor, ref)
    active = p > thr
    out = dict(first=0, last=0, p=p, active=active, thr=thr, candidates=[], segments=[], flags=[], visits=[], levels=[])
    if not active.any():
        return out
    idx = np.flatnonzero(active)
    f, l = int(idx[0]), int(idx[-1])
    first, last = max(0, HOP * (f - pad)), min(n, HOP * (l + pad) + FRAME)
    cand = []
    t = f + 1
    while t <= l:
        if active[t]:
            t += 1
            continue
        u = t
        while not active[t]:                                # (frame l is active: the run ends at or before it)
            t += 1
        v = t
        if v - u >= min_silence_frames:
            M = HOP * ((u + 3 + v) // 2)
            cand.append((min(HOP * (u + 3 + pad), M), max(HOP * (v - pad), M)))
    nc = len(cand)
    e = [c[0] for c in cand] + [last]
    s = [c[1] for c in cand] + [None]
    segments, visits = [], [0] * (nc + 1)
    cur, have, j = first, False, 0
    while j <= nc:
        visits[j] += 1
        L = e[j] - cur
        if L > max_samples and have:
            segments.append((cur, e[j - 1]))
            cur, have = s[j - 1], False
            continue
        if j == nc or L >= target_samples or L > max_samples:
            segments.append((cur, e[j]))
            cur, have = s[j], False
        else:
            have = True
        j += 1
    flags = [(OVER if b - a > max_samples else 0) | (SHORT if b - a < min_samples else 0) for a, b in segments]
    levels = []
    for a, b in segments:
        t0, t1 = -(-a // HOP), min(T, -(-b // HOP))
        pa, act = p[t0:t1], active[t0:t1]
        ns, ni = int(act.sum()), int((~act).sum())
        levels.append((ns + ni, ns, math.fsum(pa[act]) / ns if ns else 0.0, math.fsum(pa[~act]) / ni if ni else 0.0))
    out.update(first=first, last=last, candidates=cand, segments=segments, flags=flags, visits=visits, levels=levels)
    return out


def plan_batch(items, K):
    """The [B][K] outputs from the items' plans, slots at or past count zero."""
    B = len(items)
    r = dict(segments=np.zeros((B, K, 2), np.int64), flags=np.zeros((B, K), np.int32), count=np.zeros((B,), np.int32),
             wanted=np.zeros((B,), np.int32), frames=np.zeros((B, K), np.int32), speech_frames=np.zeros((B, K), np.int32),
             speech_power=np.zeros((B, K), np.float64), noise_power=np.zeros((B, K), np.float64))
    for b, it in enumerate(items):
        c = min(len(it["segments"]), K)
        r["wanted"][b], r["count"][b] = len(it["segments"]), c
        for k in range(c):
            r["segments"][b, k] = it["segments"][k]
            r["flags"][b, k] = it["flags"][k]
            r["frames"][b, k], r["speech_frames"][b, k], r["speech_power"][b, k], r["noise_power"][b, k] = it["levels"][k]
    return r


def gather(audio, plan, drop, R, S_out):
    """The rows from the batch plan (plan_batch's arrays) and the waveforms audio [B][S]."""
    r = dict(audio=np.zeros((R, S_out), np.float32), audio_len=np.zeros((R,), np.int64), item=np.full((R,), -1, np.int32),
             index=np.zeros((R,), np.int32), bounds=np.zeros((R, 2), np.int64), row_flags=np.zeros((R,), np.int32),
             rows=np.zeros((1,), np.int32), rows_wanted=np.zeros((1,), np.int32))
    row = 0
    for b in range(len(plan["count"])):
        for k in range(int(plan["count"][b])):
            fl = int(plan["flags"][b, k])
            if fl & drop:
                continue
            if row < R:
                s, e = (int(v) for v in plan["segments"][b, k])
                m = min(e - s, S_out)
                r["audio"][row, :m] = audio[b][s:s + m]
                r["audio_len"][row], r["item"][row], r["index"][row], r["bounds"][row] = m, b, k, (s, e)
                r["row_flags"][row] = fl | (CUT if e - s > S_out else 0)
            row += 1
    r["rows"][0], r["rows_wanted"][0] = min(row, R), row
    return r
