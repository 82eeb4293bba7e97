"""numpy restatement of the word-level prosody pieces, written from their definition (include/ispk.h) and
not from the kernels: the per-token control algebra of ispk_infer_features_tokens_f32 in float64, and the gain envelope of
ispk_gain_envelope_f32 (the weight w in fp32 as defined, everything else in float64)."""
import numpy as np

F32 = np.float32


def infer_features_tokens_ref(pred, duration_target, pitch_target, energy_target, controls, round_duration=False):
    """pred [B, L, 3], controls [B, L, 5] = (duration_factor, pitch_factor, pitch_delta, energy_factor, energy_delta) per token ->
    (duration [B, L], features [B, L, 2]) in float64:
      duration = max(duration_factor (exp(pred[..., 0]) - 1), 0), rounded half to even before the clamp with round_duration,
                 replaced by the target where that is >= 0
      features = [(pitch_target | pred[..., 1]) pitch_factor + pitch_delta, (energy_target | pred[..., 2]) energy_factor + energy_delta]"""
    pred, c = np.asarray(pred, np.float64), np.asarray(controls, np.float64)
    scaled = c[..., 0] * (np.exp(pred[..., 0]) - 1.0)
    d = np.maximum(np.rint(scaled) if round_duration else scaled, 0.0)
    if duration_target is not None:
        t = np.asarray(duration_target, np.float64)
        d = np.where(t < 0, d, t)
    p = pred[..., 1] if pitch_target is None else np.asarray(pitch_target, np.float64)
    e = pred[..., 2] if energy_target is None else np.asarray(energy_target, np.float64)
    return d, np.stack([p * c[..., 1] + c[..., 2], e * c[..., 3] + c[..., 4]], axis=-1)


def envelope_ref(length, marks, gain, ramp):
    """One item: marks [L, 2] (start, end), gain [L] -> (e float64 [length], stats).  A token with a negative start or end is
    dead; the others are clamped to [0, length] and live when start < end.  stats: the samples inside a ramp, those inside a
    ramp that a neighbour's half length cut short (h < ramp), the boundaries that are steps (h = 0), and the live tokens."""
    e = np.ones(length, np.float64)
    stats = dict(ramp=0, cut=0, steps=0, live=0, tail=0)
    live = []
    for (s, t), g in zip(np.asarray(marks).tolist(), np.asarray(gain, np.float64).tolist()):
        if s < 0 or t < 0:
            continue
        s, t = min(max(s, 0), length), min(max(t, 0), length)
        if s < t:
            live.append((s, t, g))
    stats["live"] = len(live)
    if not live:
        return e, stats
    assert live[0][0] == 0 and all(a[1] == b[0] for a, b in zip(live, live[1:])), "the live tokens tile [0, E)"
    for s, t, g in live:
        e[s:t] = g
    e[live[-1][1]:] = live[-1][2]
    stats["tail"] = length - live[-1][1]
    for (sj, p, gj), (_, ek, gk) in zip(live, live[1:]):
        h = min(int(ramp), (p - sj) // 2, (ek - p) // 2)
        if h == 0:
            stats["steps"] += 1
        for n in range(p - h, p + h):
            i = n - p + h
            w = F32(2 * i + 1) / F32(4 * h)                                # fp32, as defined
            e[n] = gj + (gk - gj) * float(w)
        stats["ramp"] += 2 * h
        if h < ramp:
            stats["cut"] += 2 * h
    return e, stats


def gain_envelope_ref(audio, audio_len, token_marks, token_gain, ramp):
    """audio [B, S], audio_len [B] (outside [0, S]: 0), token_marks [B, L, 2], token_gain [B, L] -> (out float64 [B, S], the
    stats of every item).  out = audio e below the length, 0 from there on."""
    audio = np.asarray(audio, np.float64)
    B, S = audio.shape
    out, stats = np.zeros((B, S), np.float64), []
    for b in range(B):
        n = int(audio_len[b])
        n = n if 0 <= n <= S else 0
        e, st = envelope_ref(n, token_marks[b], token_gain[b], ramp)
        out[b, :n] = audio[b, :n] * e
        stats.append(st)
    return out, stats
