"""GPU: the synthesis scorer (csrc/dtw.hip) - ispk_dtw_f32 bit for bit against the float64 reference (tests/dtw_reference.py) on
integer cost matrices, across batch sizes, frame counts on and around the wave edges and at the limits, ragged lengths, strides
and ties; ispk_mcd_dtw_f32 on stretched, perturbed mels and pitch tracks against float64 along its own path; the edge
behaviour; and SynthesisEvaluator end to end: no PyTorch kernel, score_infer as one HIP graph."""
import zlib

import numpy as np
import pytest
import torch

import dtw_reference as ref
from isp_tts_amd import graph, runtime, synth
from isp_tts_amd.acoustic import SynthesisEvaluator, create_dct

pytestmark = pytest.mark.gpu
DEV = "cuda"
# Relative tolerance of conditions (b), (c), (d) below and the absolute one of f0_rmse_cents: 8 x the largest deviation of the GPU
# from float64 measured over this file's cases on an MI355X, rounded up to one significant digit:
# measured 2.21e-6 (relative; the largest is a score of (d), the totals of (c) reach 1.37e-6, the paths of (b) 2e-15) and
# 9.88e-6 cents.  The ceiling for TOL is 2.5e-4 (4,096 sequential fp32 additions at 2^-24).
TOL = 2e-5
TOL_CENTS = 8e-5
MEASURED = {"path_vs_optimum": 0.0, "total_vs_resum": 0.0, "metric": 0.0, "cents": 0.0}
NAN = float("nan")


def _note(key, value):
    MEASURED[key] = max(MEASURED[key], float(value))


# ---------------------------------------------------------------------------------------------------- ispk_dtw_f32, exact
def call_dtw(cost, n_len, m_len, want_path=True, pad=8):
    """The C entry with sentinels around every output and the workspace -> (total, steps, path | None, sentinels intact)."""
    B, N, M = cost.shape
    plen = (N + M - 1) * 2
    need = runtime.dtw_workspace_floats(B, N, M)
    ws = torch.full((need + 2 * pad,), NAN, device=DEV)
    total = torch.full((B + 2,), NAN, device=DEV)
    steps = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    path = torch.full((B * plen + 4,), -9, dtype=torch.int16, device=DEV)
    rc = runtime.lib().ispk_dtw_f32(cost.data_ptr(), cost.stride(0), cost.stride(1), n_len.data_ptr(), m_len.data_ptr(),
                                    total[1:].data_ptr(), steps[1:].data_ptr(), path[2:].data_ptr() if want_path else None,
                                    ws[pad:].data_ptr(), need, B, N, M, runtime._stream())
    assert rc == 0, runtime.lib().ispk_last_error_string()
    torch.cuda.synchronize()
    intact = bool(torch.isnan(ws[:pad]).all() and torch.isnan(ws[pad + need:]).all() and torch.isnan(total[[0, -1]]).all()
                  and (steps[[0, -1]] == -7).all() and (path[:2] == -9).all() and (path[-2:] == -9).all())
    if not want_path:
        intact = intact and bool((path == -9).all())
    return total[1:-1].clone(), steps[1:-1].clone(), path[2:-2].view(B, N + M - 1, 2).clone() if want_path else None, intact


def _lengths(g, B, N, M, kind):
    n = torch.randint(1, N + 1, (B,), generator=g)
    m = torch.randint(1, M + 1, (B,), generator=g)
    if kind == "full":
        n[:], m[:] = N, M
    elif B == 1:
        m[0] = max(1, M // 2)
        n[0] = N
    else:
        n[0], m[0] = N, M                 # the padded size
        n[1], m[1] = 1, M                 # a single row
        if B > 2:
            n[2], m[2] = N, 1             # a single column
        if B > 3:
            n[3], m[3] = 1, 1
    return n, m


def _cost(g, B, N, M, kind, strided, n_len, m_len):
    """Small non-negative integers (every partial sum is exact in fp32 and float64); NaN outside each item's n x m cells and,
    when `strided`, in the gaps of a buffer with padded batch and row strides and an offset base."""
    hi = {"rand": 4, "rand9": 10, "equal": 1}[kind]
    c = torch.randint(0, hi, (B, N, M), generator=g).float() + (3.0 if kind == "equal" else 0.0)
    inside = (torch.arange(N)[None, :, None] < n_len[:, None, None]) & (torch.arange(M)[None, None, :] < m_len[:, None, None])
    c = torch.where(inside, c, torch.full_like(c, NAN))
    if not strided:
        return c.to(DEV)
    buf = torch.full((B + 1, N + 2, M + 5), NAN, device=DEV)
    v = buf[1:, 1:N + 1, 2:M + 2]
    v.copy_(c)
    return v


def _exact_matrix():
    small = [(1, 2), (2, 1), (1, 65), (65, 1), (2, 63), (63, 2), (63, 64), (64, 63), (64, 65), (65, 64), (63, 65), (65, 63)]
    mid = [(512, 63), (63, 512), (512, 65), (65, 512), (64, 512), (512, 64), (2, 512), (512, 1)]
    big = [(1723, 512), (512, 1723), (1723, 2048), (2048, 1723), (2048, 512), (512, 2048), (2048, 1), (1, 2048), (1723, 65),
           (64, 2048), (63, 1723), (2048, 2)]
    cases, i = [], 0
    for group, Bs in ((small, (1, 2, 3, 5, 64, 65)), (mid, (1, 2, 5, 33)), (big, (1, 2, 3))):
        for N, M in group:
            cases.append((Bs[i % len(Bs)], N, M, ("rand", "equal", "rand9")[i % 3], ("full", "ragged")[(i // 3) % 2], i % 4 == 1))
            i += 1
    cases += [(1, 1, 1, "rand", "full", False), (2, 64, 64, "equal", "ragged", False), (65, 65, 63, "equal", "ragged", True),
              (3, 512, 512, "equal", "full", True), (4, 512, 512, "rand", "ragged", False), (2, 1723, 1723, "equal", "ragged", False),
              (1, 1723, 1723, "rand9", "full", True), (1, 2048, 2048, "rand", "full", True), (2, 2048, 2048, "equal", "ragged", False),
              (64, 63, 65, "rand", "ragged", True), (5, 257, 300, "rand", "full", False), (5, 1025, 130, "equal", "ragged", True)]
    return cases


EXACT = _exact_matrix()


def _eid(c):
    B, N, M, kind, lens, strided = c
    return f"B{B}-{N}x{M}-{kind}-{lens}{'-strided' if strided else ''}"


def check_exact(cost, n_len, m_len):
    B, N, M = cost.shape
    total, steps, path, intact = call_dtw(cost, n_len.to(DEV), m_len.to(DEV))
    assert intact, "a store outside the outputs / the workspace"
    total, steps, path, host = total.cpu().numpy(), steps.cpu().numpy(), path.cpu().numpy(), cost.cpu().double().numpy()
    for b in range(B):
        n, m = int(n_len[b]), int(m_len[b])
        t, p = ref.dtw(host[b, :n, :m])
        assert np.float32(t) == t and total[b] == np.float32(t), (b, n, m, float(total[b]), t)
        assert steps[b] == len(p), (b, n, m, int(steps[b]), len(p))
        assert np.array_equal(path[b], ref.padded_path(p, N, M)), (b, n, m)
    return total, steps, path


@pytest.mark.parametrize("case", EXACT, ids=[_eid(c) for c in EXACT])
def test_dtw_matrix_bit_for_bit(case):
    B, N, M, kind, lens, strided = case
    g = torch.Generator().manual_seed(zlib.crc32(_eid(case).encode()))
    n_len, m_len = _lengths(g, B, N, M, lens)
    check_exact(_cost(g, B, N, M, kind, strided, n_len, m_len), n_len, m_len)


def test_dtw_without_a_path_and_through_the_wrapper():
    g = torch.Generator().manual_seed(11)
    n_len, m_len = _lengths(g, 5, 130, 97, "ragged")
    cost = _cost(g, 5, 130, 97, "rand", False, n_len, m_len)
    t0, s0, p0, ok0 = call_dtw(cost, n_len.to(DEV), m_len.to(DEV))
    t1, s1, p1, ok1 = call_dtw(cost, n_len.to(DEV), m_len.to(DEV), want_path=False)
    assert ok0 and ok1 and p1 is None and torch.equal(t0, t1) and torch.equal(s0, s1)
    t2, s2, p2 = runtime.dtw(cost, n_len.to(DEV), m_len.to(DEV))
    assert torch.equal(t0, t2) and torch.equal(s0, s2) and torch.equal(p0, p2)
    t3, s3, p3 = runtime.dtw(cost[:0], n_len[:0].to(DEV), m_len[:0].to(DEV))          # B = 0: no launch
    assert t3.shape == (0,) and s3.shape == (0,) and p3.shape == (0, 226, 2)


def test_dtw_bad_lengths_give_nan_for_that_item_only():
    g = torch.Generator().manual_seed(12)
    n_len, m_len = torch.tensor([40, 0, 41, 17, 9]), torch.tensor([50, 20, 30, 51, -3])
    ok_n, ok_m = n_len.clamp(1, 40), m_len.clamp(1, 50)
    cost = _cost(g, 5, 40, 50, "rand", False, ok_n, ok_m)
    total, steps, path, intact = call_dtw(cost, n_len.to(DEV), m_len.to(DEV))
    assert intact
    for b in (1, 2, 3, 4):
        assert torch.isnan(total[b]) and steps[b] == 0 and (path[b] == -1).all()
    t, p = ref.dtw(cost[0].cpu().double().numpy())
    assert float(total[0]) == t and int(steps[0]) == len(p) and np.array_equal(path[0].cpu().numpy(), ref.padded_path(p, 40, 50))


# ---------------------------------------------------------------------------------------------------- ispk_mcd_dtw_f32
def _layout(x, layout, lens):
    """[B, C, T] on the host -> the device view in `layout`: "bct", "btc", or "pad_bct" / "pad_btc": a view into a NaN-filled
    buffer with padded strides whose frames past each length are NaN as well."""
    if layout == "bct":
        return x.to(DEV)
    if layout == "btc":
        return x.transpose(1, 2).contiguous().to(DEV)
    B, C, T = x.shape
    x = torch.where(torch.arange(T)[None, None, :] < lens[:, None, None], x, torch.full_like(x, NAN))
    if layout == "pad_bct":
        buf = torch.full((B + 1, C + 2, T + 7), NAN, device=DEV)
        v = buf[1:, 1:C + 1, 3:T + 3]
        v.copy_(x)
        return v
    buf = torch.full((B + 2, T + 3, C + 4), NAN, device=DEV)
    v = buf[1:B + 1, 2:T + 2, 4:C + 4]
    v.copy_(x.transpose(1, 2))
    return v


def _stretched(g, tgt, m_len, lo, hi, noise):
    """A time-stretched (by a factor in [lo, hi] per item), perturbed copy of tgt [B, C, M] -> (out [B, C, N], n_len, index)."""
    B, C, M = tgt.shape
    n_len = torch.tensor([min(2048, max(1, int(round(int(m) * f)))) for m, f in zip(m_len, g.uniform(lo, hi, B))])
    N = int(n_len.max())
    out = torch.zeros(B, C, N)
    index = []
    for b in range(B):
        n, m = int(n_len[b]), int(m_len[b])
        idx = torch.from_numpy(np.minimum((np.arange(n) * m) // n, m - 1))
        out[b, :, :n] = tgt[b][:, idx] + noise * torch.from_numpy(g.standard_normal((C, n)).astype(np.float32))
        index.append(idx)
    return out, n_len, index


def _pitch_pair(g, pitch_tgt, m_len, n_len, index):
    """The output's pitch: the target's along the stretch, detuned by a few percent, with a few voicing flips."""
    B, N = len(n_len), int(n_len.max())
    out = torch.zeros(B, N)
    for b in range(B):
        n = int(n_len[b])
        p = pitch_tgt[b][index[b]].numpy().copy()
        p = p * np.exp2(g.normal(0.0, 0.03, n)).astype(np.float32)
        flip = g.random(n) < 0.05
        p = np.where(flip, np.where(p > 0, 0.0, 180.0), p).astype(np.float32)
        out[b, :n] = torch.from_numpy(p)
    return out


REAL = {
    # name: (B, M, stretch range, noise, layout of out / target, n_mfcc, pitch)
    "voices": (64, 1723, (0.8, 1.18), 0.5, ("bct", "bct"), 13, True),
    "b5-65": (5, 65, (0.6, 1.6), 0.5, ("btc", "bct"), 20, False),
    "b3-512": (3, 512, (0.7, 1.3), 0.3, ("pad_bct", "pad_btc"), 13, True),
    "b1-64": (1, 64, (1.0, 1.0), 1.0, ("bct", "btc"), 13, True),
    "b2-63": (2, 63, (0.5, 0.52), 0.2, ("pad_btc", "bct"), 2, False),
    "b7-300": (7, 300, (0.9, 1.1), 0.05, ("btc", "btc"), 80, True),
}


def _real_case(name):
    B, M, (lo, hi), noise, layouts, n_mfcc, with_pitch = REAL[name]
    g = np.random.default_rng(zlib.crc32(name.encode()))
    voices = synth.make_stats_case("voices")
    if name == "voices":
        m_len = voices["mel_len"].clone()
    else:
        m_len = torch.from_numpy(g.integers(max(1, M // 2), M + 1, B))
        m_len[0] = M
    tgt = synth.make_inputs(B, 100, M)["mel"] * (torch.arange(M)[None, None, :] < m_len[:, None, None])
    out, n_len, index = _stretched(g, tgt, m_len, lo, hi, noise)
    pitch_tgt = pitch_out = None
    if with_pitch:
        pitch_tgt = torch.zeros(B, M)
        for b in range(B):                              # ("voices": the case itself; else: the start of one of its long items)
            src = voices["pitch"][b] if name == "voices" else voices["pitch"][0, 200 * b:]
            pitch_tgt[b, :int(m_len[b])] = src[:int(m_len[b])]
        pitch_out = _pitch_pair(g, pitch_tgt, m_len, n_len, index)
    return {"out": out, "tgt": tgt, "n_len": n_len, "m_len": m_len, "pitch_out": pitch_out, "pitch_tgt": pitch_tgt,
            "layouts": layouts, "dct": create_dct(n_mfcc, 80)}


def call_mcd_dtw(mel_out, n_len, mel_tgt, m_len, dct, pitch_out=None, pitch_tgt=None, pad=8):
    """The C entry with sentinels -> (per_item [4, B], means [4], cost_out [B, N, M] (NaN where it was not written), intact)."""
    B = n_len.shape[0]
    C, n_mfcc = dct.shape
    mo, mt = runtime._mel_strides(mel_out, C), runtime._mel_strides(mel_tgt, C)
    N, M = mo[1], mt[1]
    need = runtime.mcd_dtw_workspace_floats(B, N, M, n_mfcc)
    ws = torch.full((need + 2 * pad,), NAN, device=DEV)
    out = torch.full((4 * B + 4 + 2 * pad,), NAN, device=DEV)
    items, means = out[pad:pad + 4 * B].view(4, B), out[pad + 4 * B:pad + 4 * B + 4]
    cost = torch.full((B * N * M + 2 * pad,), NAN, device=DEV)
    rc = runtime.lib().ispk_mcd_dtw_f32(
        mel_out.data_ptr(), mo[2], mo[3], mo[4], mel_tgt.data_ptr(), mt[2], mt[3], mt[4], dct.data_ptr(), n_len.data_ptr(),
        m_len.data_ptr(), runtime._ptr(pitch_out), pitch_out.stride(0) if pitch_out is not None else 0, runtime._ptr(pitch_tgt),
        pitch_tgt.stride(0) if pitch_tgt is not None else 0, ws[pad:].data_ptr(), need, items.data_ptr(), means.data_ptr(),
        cost[pad:].data_ptr(), B, C, N, M, n_mfcc, runtime._stream())
    assert rc == 0, runtime.lib().ispk_last_error_string()
    torch.cuda.synchronize()
    intact = bool(torch.isnan(ws[:pad]).all() and torch.isnan(ws[pad + need:pad + need + pad]).all() and torch.isnan(out[:pad]).all()
                  and torch.isnan(out[pad + 4 * B + 4:]).all() and torch.isnan(cost[:pad]).all() and torch.isnan(cost[-pad:]).all())
    return items.clone(), means.clone(), cost[pad:pad + B * N * M].view(B, N, M), intact


@pytest.mark.parametrize("name", list(REAL))
def test_mcd_dtw_against_float64_along_its_own_path(name):
    """For EVERY item: (a) the GPU's path (ispk_dtw_f32 on the cost matrix ispk_mcd_dtw_f32 gave out) is a warping path;
    (b) its cost re-summed in float64 over the float64 cepstral cost is within TOL of the float64 optimum; (c) the reported
    total is within TOL of that re-sum; (d) every score is within TOL (TOL_CENTS for f0_rmse_cents) of the float64 score along
    the GPU's own path.  Path identity is not asked: near-ties make it ill-posed for real-valued costs."""
    c = _real_case(name)
    B = len(c["n_len"])
    n_len, m_len = c["n_len"].to(DEV), c["m_len"].to(DEV)
    mel_out, mel_tgt = _layout(c["out"], c["layouts"][0], c["n_len"]), _layout(c["tgt"], c["layouts"][1], c["m_len"])
    dct = c["dct"].to(DEV)
    po = c["pitch_out"].to(DEV) if c["pitch_out"] is not None else None
    pt = c["pitch_tgt"].to(DEV) if c["pitch_tgt"] is not None else None
    items, means, cost, intact = call_mcd_dtw(mel_out, n_len, mel_tgt, m_len, dct, po, pt)
    assert intact, "a store outside the outputs / the workspace"
    total, steps, path, _ = call_dtw(cost, n_len, m_len)
    again, means2, _, _ = call_mcd_dtw(mel_out, n_len, mel_tgt, m_len, dct, po, pt)
    rows = [0, 1, 2, 3] if po is not None else [0, 3]
    assert torch.equal(items[rows].view(torch.int32), again[rows].view(torch.int32)), "repeat call differs"
    assert torch.equal(means[rows].view(torch.int32), means2[rows].view(torch.int32))
    if po is None:
        assert torch.isnan(items[1:3]).all() and torch.isnan(means[1:3]).all()             # (not written)
    items, total, steps, path = items.cpu().double().numpy(), total.cpu().double().numpy(), steps.cpu().numpy(), path.cpu().numpy()
    dct64 = c["dct"].double().numpy()
    for b in range(B):
        n, m = int(c["n_len"][b]), int(c["m_len"][b])
        K = int(steps[b])
        p = path[b, :K].astype(np.int64)
        assert ref.is_warping_path(p, n, m) and (path[b, K:] == -1).all(), (name, b, "(a)")
        c64 = ref.cepstral_cost(c["out"][b, :, :n].numpy(), c["tgt"][b, :, :m].numpy(), dct64)
        opt, _ = ref.dtw(c64)
        resum = ref.path_cost(c64, p)
        scale = max(opt, 1e-30)
        dev_b, dev_c = (resum - opt) / scale, abs(total[b] - resum) / scale
        _note("path_vs_optimum", abs(dev_b))
        _note("total_vs_resum", dev_c)
        assert resum >= opt * (1 - 1e-12) and dev_b <= TOL, (name, b, "(b)", resum, opt)
        assert dev_c <= TOL, (name, b, "(c)", float(total[b]), resum)
        want = ref.scores(resum, p, n, m, c["pitch_out"][b].numpy() if po is not None else None,
                          c["pitch_tgt"][b].numpy() if pt is not None else None)
        for row, key in ((0, "mcd_dtw"), (3, "length_ratio"), (2, "vuv_error")):
            if key in want:
                dev = abs(items[row, b] - want[key]) / max(abs(want[key]), 1e-30) if want[key] != 0 else abs(items[row, b])
                _note("metric", dev)
                assert dev <= TOL, (name, b, "(d)", key, float(items[row, b]), want[key])
        if po is not None:
            if np.isnan(want["f0_rmse_cents"]):
                assert np.isnan(items[1, b]), (name, b, "(d) f0")
            else:
                _note("cents", abs(items[1, b] - want["f0_rmse_cents"]))
                assert abs(items[1, b] - want["f0_rmse_cents"]) <= TOL_CENTS, (name, b, "(d) f0", items[1, b], want["f0_rmse_cents"])
    # the batch means: plain means of the per-item rows (NaN when an item's score is NaN)
    for row in rows:
        want = items[row].mean()
        got = float(means[row])
        assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= TOL * abs(want), (name, "mean", row, got, want)
    print(f"measured[{name}]: " + ", ".join(f"{k} {v:.3e}" for k, v in MEASURED.items()))


# ---------------------------------------------------------------------------------------------------- behaviour
def _small_pair(B=4, M=90, seed=3):
    g = np.random.default_rng(seed)
    m_len = torch.tensor([M, M // 2, M - 7, 1][:B])
    tgt = synth.make_inputs(B, 20, M)["mel"] * (torch.arange(M)[None, None, :] < m_len[:, None, None])
    out, n_len, index = _stretched(g, tgt, m_len, 0.8, 1.2, 0.4)
    voice = synth.make_stats_case("voices")["pitch"][0]                    # (1,723 frames: every item takes its own stretch of it)
    pitch_tgt = torch.stack([voice[300 * b:300 * b + M] for b in range(B)]) * (torch.arange(M)[None] < m_len[:, None])
    pitch_out = _pitch_pair(g, pitch_tgt, m_len, n_len, index)
    return [t.to(DEV) for t in (out, n_len, tgt, m_len, pitch_out, pitch_tgt)]


def test_bad_lengths_give_nan_for_that_item():
    out, n_len, tgt, m_len, po, pt = _small_pair()
    dct = create_dct(13, 80).to(DEV)
    good, _, _, _ = call_mcd_dtw(out, n_len, tgt, m_len, dct, po, pt)
    assert torch.isfinite(good[[0, 2, 3]]).all()            # (rows: mcd_dtw, vuv_error, length_ratio of every item)
    for bad_n, bad_m in ((0, None), (out.shape[2] + 1, None), (None, 0), (None, tgt.shape[2] + 1), (-5, None)):
        n2, m2 = n_len.clone(), m_len.clone()
        if bad_n is not None:
            n2[1] = bad_n
        if bad_m is not None:
            m2[1] = bad_m
        items, means, _, intact = call_mcd_dtw(out, n2, tgt, m2, dct, po, pt)
        assert intact and torch.isnan(items[:, 1]).all() and torch.isnan(means).all()
        keep = [0, 2, 3]
        assert torch.equal(items[:, keep].view(torch.int32), good[:, keep].view(torch.int32))


def test_no_voiced_pair_gives_a_nan_f0_and_a_finite_vuv():
    out, n_len, tgt, m_len, po, pt = _small_pair()
    dct = create_dct(13, 80).to(DEV)
    po2 = po.clone()
    po2[0] = 0.0                                        # item 0: the output is never voiced
    pt2 = pt.clone()
    pt2[2] = 0.0                                        # item 2: the target is never voiced
    items, means, _, _ = call_mcd_dtw(out, n_len, tgt, m_len, dct, po2, pt2)
    assert torch.isnan(items[1, [0, 2]]).all() and torch.isfinite(items[2]).all() and torch.isfinite(items[[0, 3]]).all()
    assert torch.isfinite(items[1, 1]) and float(items[2, 0]) > 0 and torch.isnan(means[1]) and torch.isfinite(means[[0, 2, 3]]).all()


def test_identical_inputs_give_zero_and_the_diagonal():
    out, n_len, tgt, m_len, po, pt = _small_pair()
    dct = create_dct(13, 80).to(DEV)
    items, means, cost, _ = call_mcd_dtw(tgt, m_len, tgt.clone(), m_len, dct, pt, pt.clone())
    assert (items[0] == 0).all() and (items[2] == 0).all() and (items[3] == 1).all() and float(means[0]) == 0.0
    voiced_somewhere = (pt > 0).any(dim=1)
    assert (items[1][voiced_somewhere] == 0).all() and torch.isnan(items[1][~voiced_somewhere]).all()
    total, steps, path, _ = call_dtw(cost, m_len, m_len)
    assert torch.equal(steps.cpu(), m_len.cpu().int()) and (total == 0).all()
    for b in range(len(m_len)):
        k = int(m_len[b])
        diag = torch.arange(k, dtype=torch.int16, device=DEV)
        assert torch.equal(path[b, :k, 0], diag) and torch.equal(path[b, :k, 1], diag) and (path[b, k:] == -1).all()


def test_evaluator_keys_views_and_repeat_calls():
    out, n_len, tgt, m_len, po, pt = _small_pair()
    ev = SynthesisEvaluator()
    m = ev(out, n_len, tgt, m_len, po, pt)
    assert list(m) == ["metrics/mcd_dtw_13", "metrics/f0_rmse_cents", "metrics/vuv_error", "metrics/length_ratio"]
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in m.values())
    assert len({v.untyped_storage().data_ptr() for v in m.values()}) == 1                 # one device buffer behind all four
    m2 = ev(out, n_len, tgt, m_len, po, pt)
    assert all(torch.equal(m[k].view(torch.int32), m2[k].view(torch.int32)) for k in m)
    per = ev(out, n_len, tgt, m_len, po, pt, per_item=True)
    assert all(v.shape == (4,) for v in per.values())
    for k in m:
        mean = float(per[k].double().mean())
        assert (mean != mean and bool(torch.isnan(m[k]))) or abs(mean - float(m[k])) <= 1e-6 * abs(float(m[k])), k
    plain = ev(out, n_len, tgt, m_len)
    assert list(plain) == ["metrics/mcd_dtw_13", "metrics/length_ratio"]
    assert torch.equal(plain["metrics/mcd_dtw_13"], m["metrics/mcd_dtw_13"])
    btc = ev(out.transpose(1, 2).contiguous(), n_len, tgt, m_len)                          # the layout rule of MCD
    assert torch.equal(btc["metrics/mcd_dtw_13"], m["metrics/mcd_dtw_13"])
    m20 = SynthesisEvaluator(n_mfcc=20)(out, n_len, tgt, m_len)
    assert list(m20) == ["metrics/mcd_dtw_20", "metrics/length_ratio"] and torch.isfinite(m20["metrics/mcd_dtw_20"])
    assert not torch.equal(m20["metrics/mcd_dtw_20"], m["metrics/mcd_dtw_13"])
    empty = ev(out[:0], n_len[:0], tgt[:0], m_len[:0])                                    # B = 0: NaN means without a launch
    assert all(torch.isnan(v) for v in empty.values())


# ---------------------------------------------------------------------------------------------------- end to end
def _model():
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    return model.to(DEV).requires_grad_(False)


def _vocoder_and_features():
    from isp_tts_amd.data import AcousticFeatures
    from isp_tts_amd.vocoder import Vocoder
    voc = Vocoder.from_state_dict(synth.make_vocoder_state_dict(synth.VOCODER_DIMS["official"])).to(DEV).eval()
    return voc, AcousticFeatures(pitch_mean=0.0, pitch_std=1.0)


def _infer_inputs():
    inp = synth.make_inputs(3, 40, 96, variable=True, seed=21)
    pitch_hz = synth.make_stats_case("voices")["pitch"][:3, :96] * (torch.arange(96)[None] < inp["mel_len"][:, None])
    inputs = {"text": inp["text"].to(DEV), "text_len": inp["text_len"].to(DEV), "mel": inp["mel"].to(DEV),
              "mel_len": inp["mel_len"].to(DEV), "pitch_hz": pitch_hz.to(DEV)}
    kwargs = {"duration_target": torch.full((3, 40), 2, dtype=torch.int64, device=DEV), "steps": 4,
              "flow_noise": inp["flow_x0"].to(DEV), "max_dec_len": 80}
    return inputs, kwargs


def test_score_infer_matches_the_pieces():
    model = _model()
    voc, feats = _vocoder_and_features()
    inputs, kw = _infer_inputs()
    ev = SynthesisEvaluator()
    got = ev.score_infer(model, inputs, voc, feats, **kw)
    mel, ao = model.infer(inputs["text"], text_lengths=inputs["text_len"], **kw)
    audio, alen = voc(mel, ao.dec_lengths)
    pitch = feats(audio, alen)["pitch"]
    want = ev(mel, ao.dec_lengths, inputs["mel"], inputs["mel_len"], pitch, inputs["pitch_hz"])
    assert list(got) == list(want) and len(got) == 4
    assert all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in got)
    assert torch.isfinite(got["metrics/mcd_dtw_13"]) and torch.isfinite(got["metrics/vuv_error"])
    plain = ev.score_infer(model, inputs, **kw)
    assert list(plain) == ["metrics/mcd_dtw_13", "metrics/length_ratio"]
    assert torch.equal(plain["metrics/mcd_dtw_13"], got["metrics/mcd_dtw_13"])
    want_ratio = (ao.dec_lengths.double() / inputs["mel_len"].double()).mean()
    assert abs(float(plain["metrics/length_ratio"]) - float(want_ratio)) < 1e-6
    with pytest.raises(ValueError, match="Hz"):
        from isp_tts_amd.data import AcousticFeatures
        ev.score_infer(model, inputs, voc, AcousticFeatures(pitch_mean=120.0, pitch_std=30.0), **kw)
    with pytest.raises(ValueError, match="both"):
        ev.score_infer(model, inputs, voc, None, **kw)


def test_evaluator_and_score_infer_issue_no_aten_compute_ops():
    """Both calls are libispk launches only: the spy of tests/test_gpu_metrics.py sees views and allocations on the device."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream", "aten.view_as")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = str(func)
            if not name.startswith(harmless):
                if any(t.is_cuda for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)):
                    seen.append(name)
            return out

    out, n_len, tgt, m_len, po, pt = _small_pair()
    model = _model()
    voc, feats = _vocoder_and_features()
    inputs, kw = _infer_inputs()
    ev = SynthesisEvaluator()
    ev(out, n_len, tgt, m_len, po, pt)                  # (the first calls put the DCT basis and the staged weights on the device)
    ev.score_infer(model, inputs, voc, feats, **kw)
    torch.cuda.synchronize()
    with Spy():
        a = ev(out, n_len, tgt, m_len, po, pt)
        b = ev(out, n_len, tgt, m_len, per_item=True)
        c = ev.score_infer(model, inputs, voc, feats, **kw)
        d = ev.score_infer(model, inputs, **kw)
    torch.cuda.synchronize()
    assert seen == [], f"PyTorch kernels inside the synthesis evaluator: {sorted(set(seen))}"
    assert all(torch.isfinite(v).all() for m in (a, b, d) for v in m.values()) and torch.isfinite(c["metrics/mcd_dtw_13"])


@pytest.mark.parametrize("with_audio", [False, True])
def test_score_infer_as_one_graph(with_audio):
    """text -> mel (-> waveform -> pitch) -> scores captured as ONE HIP graph: the replays equal the eager call bit for bit."""
    model = _model()
    voc, feats = _vocoder_and_features() if with_audio else (None, None)
    inputs, kw = _infer_inputs()
    ev = SynthesisEvaluator()
    eager = {k: v.clone() for k, v in ev.score_infer(model, inputs, voc, feats, **kw).items()}
    torch.cuda.synchronize()
    assert len(eager) == (4 if with_audio else 2)
    g = graph.GraphedCall(lambda: ev.score_infer(model, inputs, voc, feats, **kw))
    for _ in range(2):
        for v in g.out.values():
            v.fill_(NAN)
        replayed = g.replay()
        torch.cuda.synchronize()
        for k, v in eager.items():
            assert torch.equal(replayed[k].view(torch.int32), v.view(torch.int32)), k
    assert torch.isfinite(eager["metrics/mcd_dtw_13"]) and torch.isfinite(eager["metrics/length_ratio"])
