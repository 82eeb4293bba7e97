"""The true-peak look-ahead limiter on the GPU (ispk_limit_f32, data.Limiter, AudioConditioner(limiter=), Synthesizer(limiter=))
against the float64 reference (tests/limiter_reference.py), and bit for bit where the contract says so.

Bound, per item, with A = max |g x| of the item, c the ceiling and H = max_p sum_k |h[p][k]| (1.864) of the table:
    |out - ref64| <= (13 * 2^-24 * H * A / c + 4 * 2^-24) * A
The 12-tap fp32 dot of fp32(g x) is 13 roundings of 2^-24 on terms that sum to at most H A, so |e - e64| <= 13 * 2^-24 * H * A; r =
c / e with e > c moves by at most that over c (relative to r <= 1), and the output by A times it; the division, the product
with s and the casts are the four further roundings.  The smoothing sum is float64 in the kernel and adds nothing that shows.
true_peak and reduction are held to the same bound relative to their own value.  3.0e-6 A at the A / c = 1.9 used here.
Measured on an MI355X over the cases below, every look-ahead alike: worst |out - ref64| 0.079 of the bound, true_peak 0.24 and
reduction 0.03 of theirs (the tests print the figures; DESIGN.md 4.27 records them)."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import limiter_reference as R
from isp_tts_amd import data, longform, runtime, synth
from isp_tts_amd.data import AudioConditioner, Limiter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS = runtime.LIMIT_TILE_SAMPLES
C = float(np.float32(10.0 ** (-1.0 / 20.0)))
LOOKAHEADS = [1, 8, 33, 256]
ITEM_LENS = [0, 1, 5, 6, TS - 1, TS, TS + 1, 2 * TS + 40]
S_C, LD_C = 2 * TS + 64, 2 * TS + 72                                       # room for an odd start; a row stride above S
ROW_LENS = ITEM_LENS + [-1, S_C + 1]                                       # two rows whose length counts as 0
B_C = len(ROW_LENS)
H_MAX = float(np.abs(R.taps()).sum(axis=1).max())
U = 2.0 ** -24


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def bound_of(A):
    return (13.0 * U * H_MAX * A / C + 4.0 * U) * A


class Spy(TorchDispatchMode):
    """Records every ATen op that touches a GPU tensor, views and allocations apart."""
    HARMLESS = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.slice", "aten.select", "aten.detach", "aten.alias",
                "aten.is_", "aten.size", "aten.stride", "aten.sym_", "aten.empty_like", "aten.new_empty")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_flatten
        out = func(*args, **(kwargs or {}))
        if not str(func).startswith(self.HARMLESS):
            if any(t.is_cuda for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)):
                self.seen.append(str(func))
        return out


# ------------------------------------------------------------------------------------------------ the cases
def _items(kind, level=1.9):
    """One item per row, float64, item coordinates, scaled so that max |item| = level * c (<= 2 c).  kind: "sketch" - the three
    signals of the reference in turn; "imp4095" / "imp4096" - one impulse at that sample over a quiet background: the gain dip
    of the second spans two tiles."""
    out = []
    for b, n in enumerate(ITEM_LENS):
        if kind == "sketch":
            sig = R.signals(n, C, seed=10 + b)[("sine", "noise", "burst")[b % 3]] if n else np.zeros(0)
            top = np.abs(sig).max(initial=0.0)
            out.append(sig * (level * C / top if top > 0 else 1.0))
        else:
            sig = 0.05 * np.random.default_rng(40 + b).standard_normal(n)
            pos = int(kind[3:])
            if pos < n:
                sig[pos] = level * C
            out.append(sig)
    return out + [np.zeros(0), np.zeros(0)]


_CASES = {}


def case(kind, with_gain, with_bounds):
    """The inputs of one call (made once, on the host and on the device): NaN wherever the kernel has no business reading."""
    key = (kind, with_gain, with_bounds)
    if key in _CASES:
        return _CASES[key]
    items = _items(kind)
    g = np.random.default_rng(3).uniform(0.5, 2.0, B_C).astype(np.float32) if with_gain else None
    audio = np.full((B_C, LD_C), np.nan, np.float32)
    lens, bounds = np.array(ROW_LENS, np.int64), None
    if with_bounds:
        bounds = np.zeros((B_C, 2), np.int64)
        lens = np.array([S_C] * len(ITEM_LENS) + [-1, S_C + 1], np.int64)
    for b, it in enumerate(items):
        start = 2 * b + 1 if with_bounds else 0                            # odd: no 16-byte alignment of the first kept sample
        audio[b, start:start + len(it)] = (it / (g[b] if with_gain else 1.0)).astype(np.float32)
        if with_bounds:
            bounds[b] = (start, start + len(it))
    if with_bounds:
        bounds[-2:] = [(1, 100), (1, 100)]                                 # good bounds, but the row's length counts as 0
    c = dict(audio=audio, lens=lens, gain=g, bounds=bounds, audio_d=dev(audio)[:, :S_C], lens_d=dev(lens),
             gain_d=None if g is None else dev(g), bounds_d=None if bounds is None else dev(bounds), refs={})
    assert c["audio_d"].stride(0) == LD_C
    _CASES[key] = c
    return c


def reference(c, L):
    if L not in c["refs"]:
        c["refs"][L] = R.limit_ref(c["audio"][:, :S_C], c["lens"], c["gain"], c["bounds"], C, L)
    return c["refs"][L]


def run(c, L, rows=slice(None), out=None):
    taps = dev(data.true_peak_taps(), np.float32)
    sub = lambda t: None if t is None else t[rows]                         # noqa: E731
    r = runtime.limit(c["audio_d"][rows], sub(c["lens_d"]), taps, C, L, sub(c["gain_d"]), sub(c["bounds_d"]), out=out)
    torch.cuda.synchronize()
    return r


def apply_bits(c):
    """What ispk_audio_apply_f32 gives with the same gain and bounds (bounds (0, len) where the case has none)."""
    b = c["bounds"]
    if b is None:
        n = np.where((c["lens"] < 0) | (c["lens"] > S_C), 0, c["lens"])
        b = np.stack([np.zeros_like(n), n], axis=1)
    else:
        b = b.copy()
        b[-2:] = 0
    out, _ = runtime.audio_apply(c["audio_d"], dev(b), c["gain_d"])
    torch.cuda.synchronize()
    return host(out)


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("L", LOOKAHEADS)
def test_against_float64(L):
    worst = worst_tp = worst_red = 0.0
    for kind in ("sketch", "imp4095", "imp4096"):
        for with_gain in (False, True):
            for with_bounds in (False, True):
                c = case(kind, with_gain, with_bounds)
                tag = f"L={L} {kind} gain={with_gain} bounds={with_bounds}"
                ref, ref_len, ref_tp, ref_red, ref_s = reference(c, L)
                full = torch.full((B_C, LD_C), 7.0, device=DEV)
                out, out_len, tp, red = run(c, L, out=full[:, :S_C])
                got, tp, red = host(out), host(tp), host(red)
                assert np.array_equal(host(out_len), ref_len), tag                     # integers: exact
                assert bits(full[:, S_C:]) == bits(torch.full((B_C, LD_C - S_C), 7.0))  # nothing behind column S is written
                assert np.isfinite(got).all(), tag                                     # no NaN: nothing outside an item was read
                plain = apply_bits(c)
                for b in range(B_C):
                    n = int(ref_len[b])
                    assert not got[b, n:].any(), (tag, b)                              # zeros past every length
                    assert np.abs(got[b]).max(initial=0.0) <= np.float32(C), (tag, b)   # the ceiling, exactly
                    if n == 0:
                        assert tp[b] == 0.0 and red[b] == 1.0, (tag, b)
                        continue
                    lo = int(c["bounds"][b, 0]) if with_bounds else 0
                    gx = (1.0 if c["gain"] is None else np.float64(c["gain"][b])) * c["audio"][b, lo:lo + n].astype(np.float64)
                    A = float(np.abs(gx).max())
                    assert A / C <= 2.0, (tag, b, A / C)
                    err = float(np.abs(got[b, :n] - ref[b, :n]).max())
                    rel = bound_of(A) / A if A > 0 else 4.0 * U
                    err_tp, err_red = abs(float(tp[b]) - ref_tp[b]), abs(float(red[b]) - ref_red[b])
                    if A > 0:
                        worst = max(worst, err / bound_of(A))
                        worst_tp, worst_red = max(worst_tp, err_tp / (rel * ref_tp[b])), max(worst_red, err_red / (rel * ref_red[b]))
                    assert err <= bound_of(A), (tag, b, err, bound_of(A))
                    assert err_tp <= rel * ref_tp[b] and err_red <= rel * ref_red[b], (tag, b, err_tp, err_red, rel)
                    # untouched stretches: the bits of the apply pass
                    same = ref_s[b] == 1.0
                    assert got[b, :n][same].tobytes() == plain[b, :n][same].tobytes(), (tag, b)
                # the cases do what they are for
                if kind == "sketch":
                    assert (ref_red[4:8] < 0.6).all() and ref_red[0] == 1.0, tag
                else:
                    pos = int(kind[3:])
                    hit = [b for b in range(len(ITEM_LENS)) if ITEM_LENS[b] > pos]
                    assert hit and all(0.5 < ref_red[b] < 0.56 for b in hit), (tag, ref_red)
                    assert all((ref_s[b][pos - 1] < 1.0) and (ref_s[b][min(pos + 1, ITEM_LENS[b] - 1)] < 1.0) for b in hit[1:])
    print(f"L={L}: worst |out - ref| {worst:.3f} of the bound, true_peak {worst_tp:.3f}, reduction {worst_red:.3f} of theirs")


def test_quiet_signal_is_the_apply_pass():
    """A signal whose true peak stays below the ceiling comes out with the bits of ispk_audio_apply_f32, reduction 1.0."""
    items = _items("sketch", level=0.4)                                    # times 1.25: sample peaks at half the ceiling
    audio = np.zeros((B_C, S_C), np.float32)
    for b, it in enumerate(items):
        audio[b, :len(it)] = it.astype(np.float32)
    lens = np.array(ROW_LENS, np.int64)
    g = np.full(B_C, 1.25, np.float32)
    c = dict(audio=audio, lens=lens, gain=g, bounds=None, audio_d=dev(audio), lens_d=dev(lens), gain_d=dev(g), bounds_d=None)
    for L in (1, 256):
        out, out_len, tp, red = run(c, L)
        assert bits(out) == apply_bits(c).tobytes()
        assert (host(red) == 1.0).all() and 0.0 < float(tp.max()) < C
        assert np.array_equal(host(out_len), np.where((lens < 0) | (lens > S_C), 0, lens))


@pytest.mark.parametrize("L", [8, 256])
def test_batch_independence_and_determinism(L):
    c = case("sketch", True, True)
    out, out_len, tp, red = run(c, L)
    again = run(c, L)
    for x, y in zip((out, out_len, tp, red), again):
        assert bits(x) == bits(y)
    for b in (1, 5, 7):
        n = int(out_len[b])
        # alone
        o1, n1, t1, r1 = run(c, L, rows=slice(b, b + 1))
        assert bits(o1[0]) == bits(out[b]) and int(n1[0]) == n and bits(t1) == bits(tp[b:b + 1]) and bits(r1) == bits(red[b:b + 1])
        # at another S and an odd row stride (no 16-byte access anywhere), beside another item
        S2, LD2 = S_C + 3, S_C + 7
        a2 = torch.zeros((2, LD2), device=DEV)
        a2[:, :S_C] = c["audio_d"][[b, 4]]
        torch.nan_to_num_(a2)
        full = torch.full((2, LD2), 7.0, device=DEV)
        o2, n2, t2, r2 = runtime.limit(a2[:, :S2], dev([S2, S2], np.int64), dev(data.true_peak_taps(), np.float32), C, L,
                                       c["gain_d"][[b, 4]], c["bounds_d"][[b, 4]], out=full[:, :S2])
        torch.cuda.synchronize()
        assert bits(o2[0, :S_C]) == bits(out[b]) and not host(o2[0, S_C:]).any() and int(n2[0]) == n
        assert bits(t2[:1]) == bits(tp[b:b + 1]) and bits(r2[:1]) == bits(red[b:b + 1])
        assert bits(full[:, S2:]) == bits(torch.full((2, LD2 - S2), 7.0))


def test_measure_only():
    lim = Limiter(22050)
    assert lim.lookahead == 33
    c = case("sketch", True, False)
    _, _, tp, _ = run(c, lim.lookahead)
    got = lim.true_peak(c["audio_d"], c["lens_d"], c["gain_d"])
    torch.cuda.synchronize()
    assert got.shape == (B_C,) and got.dtype == torch.float32 and bits(got) == bits(tp)
    r = runtime.limit(c["audio_d"], c["lens_d"], lim.device_tables(DEV), C, 33, c["gain_d"], measure_only=True)
    assert r[0] is None and r[1] is None and r[3] is None and bits(r[2]) == bits(tp)
    with pytest.raises(ValueError, match="measure_only"):
        runtime.limit(c["audio_d"], c["lens_d"], lim.device_tables(DEV), C, 33, measure_only=True, out=torch.empty((B_C, S_C), device=DEV))
    # the class: the dict, its own buffers, no ATen op
    out = lim.empty_outputs(B_C, S_C, DEV)
    spy = Spy()
    with spy:
        r = lim(c["audio_d"], c["lens_d"], gain=c["gain_d"], out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert r is out and set(r) == {"audio", "audio_len", "true_peak", "reduction"} and bits(r["true_peak"]) == bits(tp)
    for kw, match in ((dict(lookahead=0), "lookahead"), (dict(lookahead=257), "lookahead"), (dict(ceiling=0.0), "ceiling")):
        args = dict(ceiling=C, lookahead=33)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            runtime.limit(c["audio_d"], c["lens_d"], lim.device_tables(DEV), args["ceiling"], args["lookahead"])
    with pytest.raises(runtime.IspkError, match="alias"):
        runtime.limit(c["audio_d"], c["lens_d"], lim.device_tables(DEV), C, 33, out=c["audio_d"])


# ------------------------------------------------------------------------------------------------ the conditioner
def test_conditioner_with_limiter():
    """A quiet clip with sparse peaks: at -14 LUFS today's gain is capped by the sample peak; with a limiter it is not."""
    rate, S = 22050, 33000
    g = np.random.default_rng(77)
    audio = np.zeros((2, S), np.float32)
    for b, n in enumerate((30000, 22050)):
        x = 0.04 * g.standard_normal(n)
        x[g.integers(2000, n - 5000, 12)] = 0.3 * np.sign(g.standard_normal(12))
        audio[b, 1500:1500 + n - 3000] = x[:n - 3000].astype(np.float32)                # silence at both ends: the trim moves
    lens = np.array([30000, 22050], np.int64)
    a_d, n_d = dev(audio), dev(lens)
    lim = Limiter(rate)
    today = AudioConditioner(rate, target_lufs=-14.0)
    r0 = today(a_d, n_d)
    torch.cuda.synchronize()
    assert set(r0) == {"audio", "audio_len", "bounds", "loudness", "peak", "gain"}
    # limiter=None: the measure and apply passes as they were, bit for bit
    b_, l_, p_, g_ = runtime.audio_measure(a_d, n_d, today.device_tables(DEV), rate, today.trim_mode, today.trim_threshold,
                                           today.pad_frames, 1, -14.0, today.peak_limit)
    o_, ol_ = runtime.audio_apply(a_d, b_, g_)
    torch.cuda.synchronize()
    for k, t in (("bounds", b_), ("loudness", l_), ("peak", p_), ("gain", g_), ("audio", o_), ("audio_len", ol_)):
        assert bits(r0[k]) == bits(t), k
    cond = AudioConditioner(rate, target_lufs=-14.0, limiter=lim)
    spy = Spy()
    out = cond.empty_outputs(2, S, DEV)
    cond.device_tables(DEV)
    with spy:
        r = cond(a_d, n_d, out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert set(r) == set(r0) | {"true_peak", "reduction"}
    for k in ("bounds", "loudness", "peak"):
        assert bits(r[k]) == bits(r0[k]), k
    loud, gain, capped = host(r["loudness"]), host(r["gain"]), host(r0["gain"])
    want = 10.0 ** ((-14.0 - loud) / 20.0)
    print(f"loudness {loud}, gain {gain} (capped today: {capped}), true_peak {host(r['true_peak'])}, reduction {host(r['reduction'])}")
    assert np.abs(gain / want - 1.0).max() <= 4.0 * U                      # the loudness gain itself
    assert (capped < 0.99 * gain).all() and np.abs(capped * host(r0["peak"]) / today.peak_limit - 1.0).max() <= 4.0 * U
    bounds = host(r["bounds"])
    assert (bounds[:, 0] > 0).all() and (bounds[:, 1] < lens).all()
    ref, ref_len, ref_tp, ref_red, _ = R.limit_ref(audio, lens, gain, bounds, C, lim.lookahead)
    got = host(r["audio"])
    assert np.array_equal(host(r["audio_len"]), ref_len)
    for b in range(2):
        A = float(gain[b]) * float(np.abs(audio[b]).max())
        assert 1.0 < A / C <= 2.0
        assert np.abs(got[b] - ref[b]).max() <= bound_of(A)
        rel = bound_of(A) / A
        assert abs(host(r["true_peak"])[b] - ref_tp[b]) <= rel * ref_tp[b] and abs(host(r["reduction"])[b] - ref_red[b]) <= rel * ref_red[b]
        assert ref_red[b] < 0.95 and np.abs(got[b]).max() <= np.float32(C)


# ------------------------------------------------------------------------------------------------ the Synthesizer
B_S, L_S, M_S, D_S, W_S = 4, 16, 128, 2, 5
BASE_FACTOR = 3.0


@pytest.fixture(scope="module")
def hifigan():
    from isp_tts_amd.hifigan import HifiGan
    return HifiGan.from_state_dict(synth.make_hifigan_state_dict(), synth.HIFIGAN_DIMS["v1"]).to(DEV).eval()


def test_synthesizer_with_limiter(gpu_model, hifigan):
    S_out = 70000
    kw = dict(batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=S_out, steps=4, fade=64, marks=True, words=W_S,
              prosody=True, ramp=128)
    inp = synth.make_inputs(B_S, L_S, M_S, variable=False, seed=44)
    noise = inp["flow_x0"].to(DEV).clone()
    noise[..., 0] += 1.0
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)         # noqa: E731
    text, tl, doc, pos, pause = inp["text"].to(DEV), inp["text_len"].to(DEV), i64([0, 1, 0, 1]), i64([0, 0, 1, 1]), i64([500, 0, 0, 0])
    word_id = (torch.arange(L_S, device=DEV) // 3).repeat(B_S, 1)
    base = longform.make_controls(B_S, duration_factor=BASE_FACTOR, device=DEV)
    controls, gain = longform.prosody_spans(B_S, L_S, [dict(item=2, tokens=(0, L_S), gain_db=12.0)], base=base, device=DEV)
    lim = Limiter(22050)

    def call(syn):
        r = syn(text, tl, doc, pos, pause, controls, flow_noise=noise, word_id=word_id, gain=gain)
        torch.cuda.synchronize()
        return r

    plain = call(longform.Synthesizer(gpu_model, hifigan, **kw))
    assert "true_peak" not in plain and "reduction" not in plain
    before = {k: host(plain[k]).copy() for k in ("audio", "audio_len", "pcm", "token_marks", "word_marks")}
    syn = longform.Synthesizer(gpu_model, hifigan, limiter=lim, **kw)
    r = call(syn)
    assert set(r) == set(plain) | {"true_peak", "reduction"}
    got = {k: r[k].clone() for k in r if r[k] is not None}
    # a replay equals the eager chain over the same static buffers, for every key
    eager = syn._chain()
    torch.cuda.synchronize()
    for k in got:
        assert bits(eager[k]) == bits(got[k]), k
    # a replay issues no ATen op (and so no host read)
    spy = Spy()
    with spy:
        syn._graph.replay()
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    # lengths and marks are those of the chain without a limiter
    for k in ("audio_len", "token_marks", "word_marks"):
        assert np.array_equal(host(got[k]), before[k]), k
    # the limited documents are the reference's on the unlimited ones
    n = before["audio_len"]
    ref, ref_len, ref_tp, ref_red, _ = R.limit_ref(before["audio"], n, None, None, C, lim.lookahead)
    audio, pcm = host(got["audio"]), host(got["pcm"])
    clipped = int((np.abs(before["pcm"].astype(np.int32)) >= 32767).sum())
    print(f"document lengths {n.tolist()}, true_peak {host(got['true_peak'])}, reduction {host(got['reduction'])}, "
          f"samples at +-32767 without the limiter {clipped}, with it {int((np.abs(pcm.astype(np.int32)) >= 32767).sum())}")
    assert ref_tp[0] > 1.0 and clipped > 0 and ref_red[0] < 1.0             # the +12 dB item takes document 0 over full scale
    for d in range(D_S):
        A = float(np.abs(before["audio"][d]).max())
        assert np.abs(audio[d] - ref[d]).max() <= bound_of(A), d
        rel = bound_of(A) / A
        assert abs(host(got["true_peak"])[d] - ref_tp[d]) <= rel * ref_tp[d] and abs(host(got["reduction"])[d] - ref_red[d]) <= rel * ref_red[d]
        assert np.abs(audio[d]).max() <= np.float32(C)
    # PCM16 sits at +-32767 no more often than the reference's output reaches what rounds there (never, under a -1 dB ceiling)
    at_rail = int((np.abs(ref) * 32768.0 >= 32766.5).sum())
    assert int((np.abs(pcm.astype(np.int32)) >= 32767).sum()) <= at_rail == 0
