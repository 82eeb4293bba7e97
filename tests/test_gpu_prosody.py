"""Word-level prosody on the GPU: the per-token control kernel (ispk_infer_features_tokens_f32), the model with [B, L, 5] controls,
the gain envelope (ispk_gain_envelope_f32) and Synthesizer(prosody=True), against the numpy references (tests/prosody_reference.py,
tests/marks_reference.py) and against the per-item forms, bit for bit where the contract says so.

Bounds.  Tokens kernel: |got - ref64| <= 1e-6 of the operands' magnitude - df (exp(x) + 1) for a duration (expf within two ulp
of exp(x), the subtraction and the product one rounding each: below 4e-7 of that), |p pf| + |pd| for a feature (two roundings).
With rounding to integers a prediction within 1e-5 of a tie may fall to either side and is left out of the comparison (the test
asserts that this leaves out less than one value in a hundred).  Envelope: |out - ref64| <= 1e-6 max|g| max|x| per call; w, the
difference, its product with w, the sum and the product with the sample are five roundings of 2^-24, about 3e-7 of that."""
import itertools

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import marks_reference as M
import prosody_reference as P
from isp_tts_amd import longform, runtime, synth
from isp_tts_amd.data import AudioConditioner

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = 256
TS = runtime.GAIN_TILE_SAMPLES


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


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


# ------------------------------------------------------------------------------------------------ the tokens kernel
def _tokens_inputs(L):
    g = np.random.default_rng(700 + L)
    B = 3
    pred = g.standard_normal((B, L, 3)).astype(np.float32)
    pred[..., 0] = pred[..., 0] * 0.6 + 0.8                                # durations exp - 1 around 1.2, some negative
    dur_f = g.uniform(0.0, 6.0, (B, L)).astype(np.float32)
    dur_f[g.random((B, L)) < 0.4] = -1.0                                   # negative: the prediction stays
    dur_i = g.integers(-2, 7, (B, L)).astype(np.int64)
    pitch = g.standard_normal((B, L)).astype(np.float32)
    energy = g.standard_normal((B, L)).astype(np.float32)
    rows = np.stack([g.uniform(0.5, 2.0, (B, L)), g.uniform(0.8, 1.25, (B, L)), g.uniform(-1.0, 1.0, (B, L)),
                     g.uniform(0.8, 1.25, (B, L)), g.uniform(-1.0, 1.0, (B, L))], axis=-1).astype(np.float32)
    return pred, {"none": None, "f32": dur_f, "i64": dur_i}, pitch, energy, rows


@pytest.mark.parametrize("rnd", [False, True], ids=["soft", "round"])
@pytest.mark.parametrize("L", [1, 5, 1025])
def test_tokens_kernel_against_float64_and_the_items_entry(L, rnd):
    pred, durs, pitch, energy, rows = _tokens_inputs(L)
    B = 3
    pred_d, rows_d = dev(pred), dev(rows)
    item_rows = rows[:, 0, :].copy()                                       # constant over an item: the items entry's case
    const_d, item_d = dev(np.repeat(item_rows[:, None, :], L, axis=1)), dev(item_rows)
    worst_d = worst_f = 0.0
    skipped = total = 0
    for dk, use_p, use_e in itertools.product(durs, (False, True), (False, True)):
        dt = None if durs[dk] is None else dev(durs[dk])
        pt, et = dev(pitch) if use_p else None, dev(energy) if use_e else None
        tag = f"L={L} round={rnd} {dk} pitch={use_p} energy={use_e}"
        dur, feats, frames = runtime.infer_features_tokens(pred_d, dt, pt, et, rows_d, round_duration=rnd)
        torch.cuda.synchronize()
        assert dur.shape == (B, L) and feats.shape == (B, L, 2) and frames.shape == (B,) and frames.dtype == torch.int64
        ref_d, ref_f = P.infer_features_tokens_ref(pred, durs[dk], pitch if use_p else None, energy if use_e else None, rows, rnd)
        c, x = rows.astype(np.float64), pred.astype(np.float64)
        scaled = c[..., 0] * (np.exp(x[..., 0]) - 1.0)
        scale_d = c[..., 0] * (np.exp(x[..., 0]) + 1.0)
        if durs[dk] is not None:
            scale_d = np.where(durs[dk] < 0, scale_d, np.abs(durs[dk].astype(np.float64)) + 1.0)
        keep = np.ones((B, L), bool)
        if rnd:                                                            # near a tie of the rounding: either integer
            tie = np.abs(scaled - np.floor(scaled) - 0.5) < 1e-5
            keep = ~tie if durs[dk] is None else ~(tie & (durs[dk] < 0))
        skipped, total = skipped + int((~keep).sum()), total + B * L
        err_d = np.abs(host(dur) - ref_d) / scale_d
        worst_d = max(worst_d, float(err_d[keep].max(initial=0.0)))
        p = (pitch if use_p else pred[..., 1]).astype(np.float64)
        q = (energy if use_e else pred[..., 2]).astype(np.float64)
        scale_f = np.stack([np.abs(p * c[..., 1]) + np.abs(c[..., 2]), np.abs(q * c[..., 3]) + np.abs(c[..., 4])], axis=-1)
        err_f = np.abs(host(feats) - ref_f) / scale_f
        worst_f = max(worst_f, float(err_f.max()))
        assert err_d[keep].max(initial=0.0) <= 1e-6 and err_f.max() <= 1e-6, (tag, worst_d, worst_f)
        # frames_wanted: the regulators' value for the kernel's own durations, exactly
        assert np.array_equal(host(frames), M.frames_from_sums(host(dur), None, rnd)), tag
        # rows constant over an item: the bits of the items entry, all three outputs
        d_c, f_c, n_c = runtime.infer_features_tokens(pred_d, dt, pt, et, const_d, round_duration=rnd)
        d_i, f_i, n_i = runtime.infer_features_items(pred_d, dt, pt, et, item_d, round_duration=rnd)
        assert bits(d_c) == bits(d_i) and bits(f_c) == bits(f_i) and bits(n_c) == bits(n_i), tag
        # without frames_wanted: no other bit changes
        d2, f2, none = runtime.infer_features_tokens(pred_d, dt, pt, et, rows_d, round_duration=rnd, want_frames=False)
        assert none is None and bits(d2) == bits(dur) and bits(f2) == bits(feats), tag
    print(f"L={L} round={rnd}: worst duration error {worst_d:.3e}, worst feature error {worst_f:.3e} of the operands "
          f"(bound 1e-6); {skipped} of {total} values near a rounding tie left out")
    assert skipped * 100 <= total


def test_tokens_entry_refuses_bad_controls():
    pred = torch.zeros((2, 4, 3), device=DEV)
    for bad in (torch.ones((2, 4, 4), device=DEV), torch.ones((2, 5), device=DEV), torch.ones((2, 4, 5), device=DEV).double()):
        with pytest.raises(ValueError, match=r"fp32 \[2, 4, 5\]"):
            runtime.infer_features_tokens(pred, None, None, None, bad)


# ------------------------------------------------------------------------------------------------ the model
def test_model_with_per_token_controls(gpu_model):
    inp = synth.make_inputs(2, 16, 128, variable=True, seed=33)
    text, tl, noise = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV).clone()
    noise[..., 0] += 1.0                                                   # durations of several frames a token
    assert gpu_model.temporal_adaptor.soft_duration

    def infer(controls):
        mel, ao = gpu_model.infer(text, text_lengths=tl, steps=4, flow_noise=noise, max_dec_len=128, controls=controls)
        fw = gpu_model.temporal_adaptor.frames_wanted.clone()
        torch.cuda.synchronize()
        return mel.clone(), ao.duration.clone(), fw

    mel_i, dur_i, fw_i = infer(longform.make_controls(2, device=DEV))
    neutral, _ = longform.prosody_spans(2, 16, [], device=DEV)
    mel_n, dur_n, fw_n = infer(neutral)
    assert bits(mel_n) == bits(mel_i) and bits(dur_n) == bits(dur_i) and bits(fw_n) == bits(fw_i)
    slow, _ = longform.prosody_spans(2, 16, [dict(item=0, tokens=(3, 7), duration_factor=2.0)], device=DEV)
    _, dur_s, fw_s = infer(slow)
    print(f"text_len {tl.tolist()}, durations of item 0 {dur_n[0].tolist()}, frames_wanted {fw_n.tolist()} -> {fw_s.tolist()}")
    assert int(tl[0]) >= 7 and float(dur_n[0, 3:7].sum()) >= 1.0           # live tokens, and a frame or more to double
    assert bits(dur_s[0, 3:7]) == bits(2.0 * dur_n[0, 3:7])                # 2 d is exact
    keep = torch.ones((2, 16), dtype=torch.bool, device=DEV)
    keep[0, 3:7] = False
    assert bits(dur_s[keep]) == bits(dur_n[keep])
    assert int(fw_s[0]) > int(fw_n[0]) and int(fw_s[1]) == int(fw_n[1])


# ------------------------------------------------------------------------------------------------ the envelope
B_E, L_E, S_E, LD_E = 4, 8, 8192, 8200
LEN_E = [8192, 5000, 300, 0]
RAMPS = [0, 1, 128, 5000]


def _marks(shift=0):
    """Hand-made item-coordinate marks (L = 8), the tile edge at TS = 4,096:
      item 0 (8,192 samples): a 100-sample token, TWO ZERO-LENGTH tokens in a row, a token up to TS - 1, two ONE-SAMPLE tokens
              (boundaries at TS - 1, TS and TS + 1, all steps: h = 0 on both sides), a token that ends at E = 8,000 < len (the
              TAIL takes its gain), a DEAD token.  The boundary at 100 is CUT to h = 50 by the shorter neighbour.
      item 1 (5,000): a 40-sample token (h cut to 20), a boundary at TS + shift - ON the tile edge, or one sample to either side -
              whose ramp crosses the edge (h = 128, or 252 - cut - at ramp 5,000), a zero-length token, E = len, three dead tokens.
      item 2 (300): a zero-length token in front, a one-sample token, ends PAST the length (clamped: (250, 400) is cut to 50
              samples, h = 25; (400, 500) to nothing), dead tokens.
      item 3 (0 samples): the marks of item 0."""
    e = TS + shift
    m = np.full((B_E, L_E, 2), -1, np.int64)
    m[0, :7] = [(0, 100), (100, 100), (100, 100), (100, TS - 1), (TS - 1, TS), (TS, TS + 1), (TS + 1, 8000)]
    m[1, :5] = [(0, 40), (40, e), (e, 4600), (4600, 4600), (4600, 5000)]
    m[2, :6] = [(0, 0), (0, 100), (100, 101), (101, 250), (250, 400), (400, 500)]
    m[3] = m[0]
    return m


@pytest.fixture(scope="module")
def envelope_case():
    g = np.random.default_rng(2024)
    audio = np.full((B_E, LD_E), np.nan, np.float32)                       # the row padding is never read
    audio[:, :S_E] = g.uniform(-1.0, 1.0, (B_E, S_E)).astype(np.float32)
    gain = g.uniform(0.25, 2.0, (B_E, L_E)).astype(np.float32)
    return dict(audio=audio, gain=gain, audio_d=dev(audio), gain_d=dev(gain), len_d=dev(LEN_E, np.int64))


def _run(c, marks, ramp, gain=None, out=None):
    a = c["audio_d"][:, :S_E]
    if out is None:
        out = torch.full((B_E, LD_E), 7.0, device=DEV)[:, :S_E]
    r = longform.gain_envelope(a, c["len_d"], dev(marks), c["gain_d"] if gain is None else gain, ramp=ramp, out=out)
    torch.cuda.synchronize()
    assert r is out
    return out


@pytest.mark.parametrize("ramp", RAMPS)
def test_envelope_against_float64(envelope_case, ramp):
    c = envelope_case
    assert c["audio_d"][:, :S_E].stride(0) == LD_E
    for shift in (0, -1, 1):
        marks = _marks(shift)
        ref, stats = P.gain_envelope_ref(c["audio"][:, :S_E], LEN_E, marks, c["gain"], ramp)
        # the bound is not vacuous: the reference alone puts samples inside ramps, and inside ramps cut by a neighbour
        for b in range(3):
            assert stats[b]["live"] >= 2 and stats[b]["tail"] == (192 if b == 0 else 0), stats[b]
            if ramp >= 1:
                assert stats[b]["ramp"] > 0, (b, stats[b])
            if ramp >= 128:                                                # (at ramp 1 a cut ramp is a step and holds no sample)
                assert stats[b]["cut"] > 0, (b, stats[b])
        assert stats[0]["steps"] >= 3 and stats[2]["steps"] >= 2 and stats[3]["live"] == 0
        out = _run(c, marks, ramp)
        got = host(out)
        bound = 1e-6 * float(c["gain"].max()) * float(np.abs(c["audio"][:, :S_E]).max())
        err = float(np.abs(got - ref).max())
        print(f"ramp={ramp} shift={shift}: max |out - ref| {err:.3e}, bound {bound:.3e}; ramp samples per item "
              f"{[s['ramp'] for s in stats]}, of them cut {[s['cut'] for s in stats]}")
        assert np.isfinite(got).all() and err <= bound
        for b in range(B_E):
            assert not got[b, LEN_E[b]:].any()                             # silence from the length on
        assert bits(out._base[:, S_E:]) == bits(torch.full((B_E, LD_E - S_E), 7.0))      # nothing behind column S is written


@pytest.mark.parametrize("ramp", RAMPS)
def test_envelope_exact_cases(envelope_case, ramp):
    c = envelope_case
    marks = _marks()
    a = host(c["audio_d"][:, :S_E])
    below = np.arange(S_E)[None, :] < np.array(LEN_E)[:, None]
    # all gains 1: the audio's bits below the length, 0 past it;  all gains g: the bits of audio * g
    for g in (1.0, 0.37):
        out = host(_run(c, marks, ramp, gain=torch.full((B_E, L_E), g, device=DEV)))
        want = np.where(below, a * np.float32(g), np.float32(0.0)).astype(np.float32)
        assert out.tobytes() == want.tobytes(), g
    batch = _run(c, marks, ramp)
    # item 1 alone gives its batch bits
    one = torch.full((1, S_E), 7.0, device=DEV)
    longform.gain_envelope(c["audio_d"][1:2, :S_E], c["len_d"][1:2], dev(marks[1:2]), c["gain_d"][1:2], ramp=ramp, out=one)
    assert bits(one[0]) == bits(batch[1])
    # in place
    work = c["audio_d"].clone()
    r = longform.gain_envelope(work[:, :S_E], c["len_d"], dev(marks), c["gain_d"], ramp=ramp, out=work[:, :S_E])
    torch.cuda.synchronize()
    assert r.data_ptr() == work.data_ptr() and bits(work[:, :S_E]) == bits(batch)
    # out=None allocates
    assert bits(longform.gain_envelope(c["audio_d"][:, :S_E], c["len_d"], dev(marks), c["gain_d"], ramp=ramp)) == bits(batch)


@pytest.mark.parametrize("L", [256, 257, 1000])
def test_envelope_beyond_the_register_path(envelope_case, L):
    """Up to 256 tokens a wave holds every end in registers; beyond, the kernel searches global memory.  Both sides of that
    threshold: the hand-made marks padded with dead tokens give the bits of the 8-token call, and a random tiling with
    zero-length tokens, some two hundred tokens under a tile, meets the float64 bound."""
    c = envelope_case
    small = _run(c, _marks(), 128)
    pad = np.full((B_E, L, 2), -1, np.int64)
    pad[:, :L_E] = _marks()
    gpad = torch.full((B_E, L), 3.0, device=DEV)
    gpad[:, :L_E] = c["gain_d"]
    assert bits(_run(c, pad, 128, gain=gpad)) == bits(small)
    g = np.random.default_rng(L)
    marks = np.full((B_E, L, 2), -1, np.int64)
    for b, (n, live) in enumerate(zip(LEN_E, (L, L - 40, L // 2, L))):
        ends = np.sort(g.integers(0, max(n - 100, 0) + 1 if b == 0 else n + 1, live))      # item 0: E < len; equal ends: zero length
        marks[b, :live, 1] = ends
        marks[b, :live, 0] = np.concatenate([[0], ends[:-1]])
    gain = g.uniform(0.25, 2.0, (B_E, L)).astype(np.float32)
    ref, stats = P.gain_envelope_ref(c["audio"][:, :S_E], LEN_E, marks, gain, 16)
    got = host(_run(c, marks, 16, gain=dev(gain)))
    bound = 1e-6 * float(gain.max()) * float(np.abs(c["audio"][:, :S_E]).max())
    err = float(np.abs(got - ref).max())
    print(f"L={L}: max |out - ref| {err:.3e}, bound {bound:.3e}; live {[s['live'] for s in stats]}, ramp samples "
          f"{[s['ramp'] for s in stats]}, cut {[s['cut'] for s in stats]}, steps {[s['steps'] for s in stats]}")
    assert all(s["ramp"] > 0 and s["cut"] > 0 for s in stats[:3]) and stats[0]["tail"] > 0
    assert np.isfinite(got).all() and err <= bound


def test_envelope_rows_that_are_not_16_byte_aligned(envelope_case):
    """The same case from sample 1 on: S = 8,191, bases 4 bytes off a 16-byte boundary, so every access is one float."""
    c = envelope_case
    S = S_E - 1
    lens = [min(n, S) for n in LEN_E]
    marks = _marks()
    a = c["audio_d"][:, 1:S_E]
    out = torch.full((B_E, LD_E), 7.0, device=DEV)
    longform.gain_envelope(a, dev(lens, np.int64), dev(marks), c["gain_d"], ramp=128, out=out[:, 1:S_E])
    torch.cuda.synchronize()
    ref, _ = P.gain_envelope_ref(c["audio"][:, 1:S_E], lens, marks, c["gain"], 128)
    got = host(out)
    bound = 1e-6 * float(c["gain"].max()) * float(np.abs(c["audio"][:, :S_E]).max())
    assert np.abs(got[:, 1:S_E] - ref).max() <= bound
    assert (got[:, 0] == 7.0).all() and (got[:, S_E:] == 7.0).all()


def test_envelope_issues_no_aten_op_and_refuses_bad_arguments(envelope_case):
    c = envelope_case
    a, marks = c["audio_d"][:, :S_E], dev(_marks())
    out = torch.empty((B_E, S_E), device=DEV)
    spy = Spy()
    with spy:
        longform.gain_envelope(a, c["len_d"], marks, c["gain_d"], ramp=128, out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    for kw, match in ((dict(ramp=-1), "ramp"), (dict(ramp=1 << 22), "ramp"), (dict(ramp=1.5), "ramp"),
                      (dict(out=torch.empty((B_E, S_E - 1), device=DEV)), "out"), (dict(out=out.double()), "out")):
        with pytest.raises(ValueError, match=match):
            longform.gain_envelope(a, c["len_d"], marks, c["gain_d"], **kw)
    with pytest.raises(ValueError, match="token_gain"):
        longform.gain_envelope(a, c["len_d"], marks, c["gain_d"][:, :7], out=out)
    with pytest.raises(ValueError, match="token_marks"):
        longform.gain_envelope(a, c["len_d"], marks[..., 0], c["gain_d"], out=out)
    with pytest.raises(runtime.IspkError, match="overlaps"):
        longform.gain_envelope(a, c["len_d"], marks, c["gain_d"], out=c["audio_d"][:, 4:S_E + 4])


# ------------------------------------------------------------------------------------------------ the Synthesizer
B_S, L_S, M_S, D_S, W_S = 4, 16, 128, 2, 5
BASE_FACTOR = 3.0       # every item: at 0.5 the four items ask for 7, 8, 8 and 15 frames, at 3.0 for 44, 49, 49 and 90 (measured on the MI355X)
MARKS_KEYS = {"pcm", "audio", "audio_len", "wanted_len", "item_offset", "item_len", "frames_wanted", "dec_lengths", "token_marks",
              "word_marks", "duration", "item_audio_len", "item_bounds", "joined_len", "doc_bounds"}


@pytest.fixture(scope="module")
def hifigan():
    from isp_tts_amd.hifigan import HifiGan
    return HifiGan.from_state_dict(synth.make_hifigan_state_dict(), synth.HIFIGAN_DIMS["v1"]).to(DEV).eval()


def _syn_inputs():
    inp = synth.make_inputs(B_S, L_S, M_S, variable=False, seed=44)
    noise = inp["flow_x0"].to(DEV).clone()
    noise[..., 0] += 1.0                                                   # longer durations: several frames a token
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)         # noqa: E731
    # document 0 = items 0, 2; document 1 = items 1, 3: what changes item 1 does not move item 2
    return dict(text=inp["text"].to(DEV), tl=inp["text_len"].to(DEV), noise=noise, doc=i64([0, 1, 0, 1]), pos=i64([0, 0, 1, 1]),
                pause=i64([500, 0, 0, 0]), word_id=(torch.arange(L_S, device=DEV) // 3).repeat(B_S, 1))


def test_synthesizer_neutral_prosody_is_todays(gpu_model, hifigan):
    kw = dict(batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=40000, steps=4,
              item_conditioner=AudioConditioner(22050, target_lufs=None), doc_conditioner=AudioConditioner(22050), fade=64,
              marks=True, words=W_S)
    i = _syn_inputs()
    base = longform.make_controls(B_S, duration_factor=BASE_FACTOR, device=DEV)
    plain = longform.Synthesizer(gpu_model, hifigan, **kw)
    assert set(plain.out) == MARKS_KEYS and "gain" not in plain.static and plain.static["controls"].shape == (B_S, 5)
    with pytest.raises(ValueError, match="gain"):
        plain(i["text"], i["tl"], i["doc"], i["pos"], gain=torch.ones((B_S, L_S), device=DEV))
    r0 = plain(i["text"], i["tl"], i["doc"], i["pos"], i["pause"], base, flow_noise=i["noise"], word_id=i["word_id"])
    torch.cuda.synchronize()
    want = {k: r0[k].clone() for k in ("pcm", "audio_len", "token_marks", "word_marks")}
    syn = longform.Synthesizer(gpu_model, hifigan, prosody=True, ramp=128, **kw)
    assert syn.static["controls"].shape == (B_S, L_S, 5) and syn.static["gain"].shape == (B_S, L_S)
    controls, gain = longform.prosody_spans(B_S, L_S, [], base=base, device=DEV)
    for c, g in ((base, None), (controls, gain)):                          # [B, 5] copied to every token, and [B, L, 5]
        r = syn(i["text"], i["tl"], i["doc"], i["pos"], i["pause"], c, flow_noise=i["noise"], word_id=i["word_id"], gain=g)
        torch.cuda.synchronize()
        assert set(r) == MARKS_KEYS | {"item_token_marks"}
        for k in want:
            assert bits(r[k]) == bits(want[k]), k
    print(f"frames_wanted {r['frames_wanted'].tolist()}, audio_len {r['audio_len'].tolist()}")
    assert int(r["audio_len"].min()) > 0
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
    # the item marks are the marks of the items alone
    tok, _, _ = M.marks_ref(host(got["duration"]), host(i["tl"]), host(got["item_audio_len"]), HOP, M_S * HOP, False)
    assert np.array_equal(host(got["item_token_marks"]), tok)
    for bad, match in ((dict(gain=torch.ones((B_S, L_S - 1), device=DEV)), "gain"), (dict(controls=torch.ones((B_S, 3, 5), device=DEV)), "controls")):
        with pytest.raises(ValueError, match=match):
            syn(i["text"], i["tl"], i["doc"], i["pos"], **bad)


def test_synthesizer_spans(gpu_model, hifigan):
    """Word 2 of item 1 slower by 1.5, word 1 of item 2 lower by 6 dB (no conditioner: a loudness gain would spread the change)."""
    S_out = 70000
    syn = longform.Synthesizer(gpu_model, hifigan, batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=S_out, steps=4, fade=64,
                               marks=True, words=W_S, prosody=True, ramp=128)
    i = _syn_inputs()
    base = longform.make_controls(B_S, duration_factor=BASE_FACTOR, device=DEV)

    def run(spans):
        c, g = longform.prosody_spans(B_S, L_S, spans, base=base, word_id=i["word_id"], device=DEV)
        r = syn(i["text"], i["tl"], i["doc"], i["pos"], i["pause"], c, flow_noise=i["noise"], word_id=i["word_id"], gain=g)
        torch.cuda.synchronize()
        return {k: host(r[k]) for k in r}, g

    n, _ = run([])
    s, gain = run([dict(item=1, words=(2, 3), duration_factor=1.5), dict(item=2, words=(1, 2), gain_db=-6.0)])
    print(f"frames_wanted {n['frames_wanted'].tolist()} -> {s['frames_wanted'].tolist()}, item_offset {s['item_offset'].tolist()}, "
          f"item 1 word 2: {n['word_marks'][1, 2].tolist()} -> {s['word_marks'][1, 2].tolist()}, item 2 tokens 3 .. 5: "
          f"{s['item_token_marks'][2, 3:6].tolist()}")
    assert int(s["frames_wanted"].max()) <= M_S and int(s["wanted_len"].max()) <= S_out      # nothing is cut
    # the marks are the reference's on the chain's own tensors
    for r in (n, s):
        tok, wrd, _ = M.marks_ref(r["duration"], host(i["tl"]), r["item_audio_len"], HOP, M_S * HOP, False, None, r["item_offset"],
                                  host(i["doc"]), r["joined_len"], None, host(i["word_id"]), W_S)
        assert np.array_equal(r["token_marks"], tok) and np.array_equal(r["word_marks"], wrd)
        tok, _, _ = M.marks_ref(r["duration"], host(i["tl"]), r["item_audio_len"], HOP, M_S * HOP, False)
        assert np.array_equal(r["item_token_marks"], tok)
    # word 2 of item 1 is longer than in the neutral run
    length = lambda m: int(m[1] - m[0])                                    # noqa: E731
    assert length(s["word_marks"][1, 2]) > length(n["word_marks"][1, 2]) > 0
    assert length(s["item_token_marks"][1, [6, 8], [0, 1]]) > length(n["item_token_marks"][1, [6, 8], [0, 1]])
    # document 0 (items 0 and 2) differs from the neutral run only inside item 2's span plus its ramps
    assert np.array_equal(s["item_offset"][[0, 2]], n["item_offset"][[0, 2]]) and np.array_equal(s["item_token_marks"][2], n["item_token_marks"][2])
    off = int(s["item_offset"][2])
    a, e = int(s["item_token_marks"][2, 3, 0]), int(s["item_token_marks"][2, 5, 1])
    assert e - a >= 4 * 128                                                # the span is longer than both ramps
    differs = s["audio"][0] != n["audio"][0]
    assert differs[off + a:off + e].any()
    outside = differs.copy()
    outside[max(off + a - 128, 0):off + e + 128] = False
    assert not outside.any(), np.flatnonzero(outside)[:8]
    # between the ramps the document holds the neutral sample times the gain, bit for bit (the join's weight is 1 there)
    g = host(gain)[2, 3]
    assert g == np.float32(10.0 ** (-6.0 / 20.0))
    mid = slice(off + a + 128, off + e - 128)
    assert s["audio"][0][mid].tobytes() == (n["audio"][0][mid] * g).astype(np.float32).tobytes()
