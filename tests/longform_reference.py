"""numpy restatement of the long-form pieces, written from their definition (include/ispk.h) and not from
the kernels: the per-item control algebra of ispk_infer_features_items_f32, the plan of ispk_join_plan (Python ints) and the
gather of ispk_join_f32 (weights in fp32 as defined, products and sums in float64)."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ per-item controls
def infer_features_items_ref(pred, duration_target, pitch_target, energy_target, controls, round_duration=False):
    """pred [B, L, 3], controls [B, 5] = (duration_factor, pitch_factor, pitch_delta, energy_factor, energy_delta) per item ->
    (duration [B, L], features [B, L, 2]) in float64:
      duration = max(duration_factor (exp(pred[..., 0]) - 1), 0), rounded half to even before the clamp with round_duration,
                 replaced by the target where that is >= 0
      features = [(pitch_target | pred[..., 1]) pitch_factor + pitch_delta, (energy_target | pred[..., 2]) energy_factor + energy_delta]"""
    pred, c = np.asarray(pred, np.float64), np.asarray(controls, np.float64)
    scaled = c[:, 0:1] * (np.exp(pred[..., 0]) - 1.0)
    d = np.maximum(np.rint(scaled) if round_duration else scaled, 0.0)
    if duration_target is not None:
        t = np.asarray(duration_target, np.float64)
        d = np.where(t < 0, d, t)
    p = pred[..., 1] if pitch_target is None else np.asarray(pitch_target, np.float64)
    e = pred[..., 2] if energy_target is None else np.asarray(energy_target, np.float64)
    return d, np.stack([p * c[:, 1:2] + c[:, 2:3], e * c[:, 3:4] + c[:, 4:5]], axis=-1)


def frames_wanted_ref(duration, round_duration=False):
    """What the regulators report for fp32 durations [B, L] without a clamp.  Soft: the fp32 sum in token order, + 0.5f,
    truncated.  Hard: the sum of (d + 0.5f) truncated, 0 below 1."""
    d = np.asarray(duration, F32)
    out = []
    for row in d:
        if round_duration:
            f = (row + F32(0.5)).astype(F32)
            out.append(int(sum(int(v) for v in f if v >= 1.0)))
        else:
            s = F32(0.0)
            for v in row:
                s = F32(s + v)
            out.append(int(F32(s + F32(0.5))))
    return np.array(out, np.int64)


# ------------------------------------------------------------------------------------------------ the join
def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def join_plan_ref(audio_len, doc, pos, pause, S, D, S_out, bounds=None, fade=0):
    """-> dict of Python-int lists: per item b: s, n, valid, ov, adv, off (-1 dropped), h, t; order: the valid items by
    (doc, pos, b); per document: items (in order), wanted, doc_len."""
    B = len(audio_len)
    pause = [0] * B if pause is None else [int(p) for p in pause]
    s, n = [0] * B, [0] * B
    for b in range(B):
        ln = int(audio_len[b])
        ln = ln if 0 <= ln <= S else 0
        sb, eb = 0, ln
        if bounds is not None:
            sb = clamp(int(bounds[b][0]), 0, ln)
            eb = clamp(int(bounds[b][1]), sb, ln)
        s[b], n[b] = sb, eb - sb
    valid = [0 <= int(doc[b]) < D for b in range(B)]
    order = sorted((b for b in range(B) if valid[b]), key=lambda b: (int(doc[b]), int(pos[b]), b))
    items = [[b for b in order if int(doc[b]) == d] for d in range(D)]
    ov, adv, off, h, t = [0] * B, [0] * B, [-1] * B, [0] * B, [0] * B
    wanted = [0] * D
    for d in range(D):
        it = items[d]
        for k, b in enumerate(it):
            nxt = it[k + 1] if k + 1 < len(it) else None
            if pause[b] < 0 and nxt is not None:
                ov[b] = min(-pause[b], n[b] // 2, n[nxt] // 2)
            adv[b] = n[b] + min(pause[b], S_out) if pause[b] >= 0 else n[b] - ov[b]
        run = 0
        for k, b in enumerate(it):
            off[b] = run
            run += adv[b]
            prv = it[k - 1] if k > 0 else None
            t[b] = ov[b] if ov[b] > 0 else min(fade, n[b] // 2)
            h[b] = ov[prv] if prv is not None and ov[prv] > 0 else min(fade, n[b] // 2)
        wanted[d] = run
    n_out = [n[b] if valid[b] else 0 for b in range(B)]
    return dict(s=s, n=n, valid=valid, ov=ov, adv=adv, off=off, h=h, t=t, order=order, items=items, wanted=wanted,
                doc_len=[min(w, S_out) for w in wanted], item_len=n_out)


def weights_ref(n, h, t):
    """w(i) = head(i) tail(i), i < n: both ramps evaluated in fp32 as defined, their product in float64 -> float64 [n]."""
    i = np.arange(n, dtype=np.int64)
    head = np.ones(n, F32)
    tail = np.ones(n, F32)
    if h > 0:
        m = i < h
        head[m] = (2 * i[m] + 1).astype(F32) / F32(2 * h)
    if t > 0:
        m = i >= n - t
        tail[m] = (2 * (n - 1 - i[m]) + 1).astype(F32) / F32(2 * t)
    return head.astype(np.float64) * tail.astype(np.float64)


def join_ref(audio, audio_len, doc, pos, pause, D, S_out, bounds=None, gain=None, fade=0):
    """audio [B, S] -> (out float64 [D, S_out], scale float64 [D] = max |g x| over each document's items, plan)."""
    audio = np.asarray(audio)
    B, S = audio.shape
    p = join_plan_ref(audio_len, doc, pos, pause, S, D, S_out, bounds, fade)
    out = np.zeros((D, S_out), np.float64)
    scale = np.zeros(D, np.float64)
    for d in range(D):
        for b in p["items"][d]:
            n, sb, off = p["n"][b], p["s"][b], p["off"][b]
            if n == 0:
                continue
            g = F32(1.0) if gain is None else F32(gain[b])
            x = audio[b, sb:sb + n].astype(np.float64)
            scale[d] = max(scale[d], float(np.abs(np.float64(g) * x).max()))
            gw = np.float64(g) * weights_ref(n, p["h"][b], p["t"][b])
            lo, hi = off, min(off + n, p["doc_len"][d])
            if hi > lo:
                out[d, lo:hi] += gw[:hi - lo] * x[:hi - lo]
    return out, scale, p


def concat_ref(audio, audio_len, doc, pos, pause, D, S_out):
    """The plain concatenation (fade 0, every pause >= 0, no gain, no bounds): items in order with their silences -> fp32."""
    audio = np.asarray(audio, F32)
    B, S = audio.shape
    out = np.zeros((D, S_out), F32)
    for d in range(D):
        it = sorted((b for b in range(B) if int(doc[b]) == d), key=lambda b: (int(pos[b]), b))
        parts = []
        for b in it:
            ln = int(audio_len[b])
            ln = ln if 0 <= ln <= S else 0
            parts += [audio[b, :ln], np.zeros(min(int(pause[b]), S_out), F32)]
        row = np.concatenate(parts)[:S_out] if parts else np.zeros(0, F32)
        out[d, :len(row)] = row
    return out
