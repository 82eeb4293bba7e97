"""numpy restatement of the speech marks (ispk_speech_marks), written from their definition in include/ispk.h (DESIGN.md section
4.25) and not from the kernel: Python ints throughout, numpy float32 for the soft mode's sequential sum, Python floats
(IEEE doubles) for the product with the hop.  `marks_ref` also counts which clamps acted, so that a test can show that its
cases reach them."""
import math

import numpy as np

F32 = np.float32
REP_MAX = 1 << 30


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def hard_reps(d):
    """hd_reps<true> of csrc/dec_len.h: (d + 0.5f) truncated, 0 below 1 (NaN compares false), cut at 2^30."""
    f = F32(F32(d) + F32(0.5))
    if not f >= 1.0:
        return 0
    return REP_MAX if f >= REP_MAX else int(f)


def soft_sums(row, n):
    """s_0 .. s_n: the fp32 running sum in token order of d' = d if d > 0 else 0 (NaN: 0)."""
    s, out = F32(0.0), [F32(0.0)]
    for t in range(n):
        d = F32(row[t])
        s = F32(s + (d if d > 0 else F32(0.0)))
        out.append(s)
    return out


def frames_from_sums(duration, text_len=None, hard=False):
    """(int64)(s_n + 0.5f) per item, or the hard mode's C_n: what the regulators report without a clamp."""
    d = np.asarray(duration, F32)
    out = []
    for b, row in enumerate(d):
        n = len(row) if text_len is None else int(text_len[b])
        n = n if 0 <= n <= len(row) else 0
        if hard:
            out.append(sum(hard_reps(v) for v in row[:n]))
        else:
            out.append(int(F32(soft_sums(row, n)[-1] + F32(0.5))))
    return np.array(out, np.int64)


def marks_ref(duration, text_len, audio_len, hop, S=2 ** 31 - 1, hard=False, bounds=None, item_offset=None, doc=None,
              doc_len=None, doc_bounds=None, word_id=None, W=0):
    """-> (token_marks int64 [B, L, 2], word_marks int64 [B, W, 2], hits): hits counts, per step of the definition, how often
    a clamp changed a value ("len_cap": the soft mode's v >= len + 1 branch; "clamp3" .. "clamp6"; "bounds_fixed" /
    "doc_bounds_fixed": a bound that was itself clamped; "dropped"; "word_ignored")."""
    d = np.asarray(duration, F32)
    B, L = d.shape
    joined = item_offset is not None
    assert joined == (doc is not None) == (doc_len is not None) and (doc_bounds is None or joined)
    tok = np.full((B, L, 2), -1, np.int64)
    wrd = np.full((B, W, 2), -1, np.int64)
    hits = dict(len_cap=0, clamp3=0, clamp4=0, clamp5=0, clamp6=0, bounds_fixed=0, doc_bounds_fixed=0, dropped=0, word_ignored=0)

    def counted(name, v, lo, hi):
        c = clamp(v, lo, hi)
        hits[name] += c != v
        return c

    for b in range(B):
        n = L if text_len is None else int(text_len[b])
        n = n if 0 <= n <= L else 0
        ln = int(audio_len[b])
        ln = ln if 0 <= ln <= S else 0
        sb, eb = 0, ln
        if bounds is not None:
            sb = counted("bounds_fixed", int(bounds[b][0]), 0, ln)
            eb = counted("bounds_fixed", int(bounds[b][1]), sb, ln)
        if joined:
            off, dd = int(item_offset[b]), int(doc[b])
            if off < 0 or not 0 <= dd < len(doc_len):
                hits["dropped"] += 1
                continue
            dl = max(int(doc_len[dd]), 0)
            ds, de = 0, dl
            if doc_bounds is not None:
                ds = counted("doc_bounds_fixed", int(doc_bounds[dd][0]), 0, dl)
                de = counted("doc_bounds_fixed", int(doc_bounds[dd][1]), ds, dl)
        if hard:
            m, run = [0], 0
            for t in range(n):
                run += hard_reps(d[b, t])
                m.append(hop * run)
        else:
            m = []
            for s in soft_sums(d[b], n):
                v = float(s) * float(hop) + 0.5                # a double; the product is exact (24 + 21 bits)
                cap = v >= ln + 1
                hits["len_cap"] += cap
                m.append(ln if cap else math.floor(v))
        for t in range(n + 1):
            v = counted("clamp3", m[t], 0, ln)
            v = counted("clamp4", v, sb, eb) - sb
            if joined:
                v = counted("clamp5", v + off, 0, dl)
                v = counted("clamp6", v, ds, de) - ds
            m[t] = v
        for t in range(n):
            tok[b, t] = (m[t], m[t + 1])
            if word_id is not None and W > 0:
                w = int(word_id[b][t])
                if 0 <= w < W:
                    if wrd[b, w, 0] < 0:
                        wrd[b, w] = (m[t], m[t + 1])
                    else:
                        wrd[b, w] = (min(wrd[b, w, 0], m[t]), max(wrd[b, w, 1], m[t + 1]))
                else:
                    hits["word_ignored"] += 1
    return tok, wrd, hits
