"""Long-form synthesis on the GPU: the per-item control kernel against the scalar entry points and the regulators, the model
with `controls`, the document join against the numpy reference (tests/longform_reference.py), and `longform.Synthesizer`
against the eager chain.

Join audio bound: max |out - ref64| <= 1e-6 max |g x| per document - a sample is at most two products of three fp32 factors
and one add, about six roundings of 2^-24 = 3.6e-7, and the bound leaves a factor of about three over that.  Measured on the
MI355X over every case of test_join_against_the_reference: at most 9.376e-8 max |g x|, a tenth of the bound."""
import itertools

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import longform_reference as R
from isp_tts_amd import graph, longform, runtime, synth
from isp_tts_amd.data import AudioConditioner, to_pcm16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS = runtime.JOIN_TILE_SAMPLES
JOIN_BOUND = 1e-6


def bits(t):
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the items kernel
def _items_inputs(L, seed=0):
    g = np.random.default_rng(100 + L + seed)
    B = 3
    pred = g.standard_normal((B, L, 3)).astype(np.float32)
    pred[..., 0] = pred[..., 0] * 0.6 + 0.8                                # durations exp - 1 around 1.2, some negative
    dur_f = g.uniform(0.0, 6.0, (B, L)).astype(np.float32)
    dur_f[g.random((B, L)) < 0.4] = -1.0                                   # negative: the prediction stays
    dur_i = g.integers(-2, 7, (B, L)).astype(np.int64)
    pitch = g.standard_normal((B, L)).astype(np.float32)
    energy = g.standard_normal((B, L)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)                              # noqa: E731
    return t(pred), {"none": None, "f32": t(dur_f), "i64": t(dur_i)}, t(pitch), t(energy)


ROWS = [(1.0, 1.0, 0.0, 1.0, 0.0), (1.37, 0.9, 0.25, 1.1, -0.3), (0.71, 1.2, -1.5, 0.8, 0.05)]


def _regulated_len(duration, rnd):
    """dec_len of the regulator that consumes `duration`, with no clamp."""
    B, L = duration.shape
    x = torch.zeros((B, L, 256), device=DEV)
    if rnd:
        return runtime.hard_regulate(x, duration, 8)[1]
    return runtime.length_regulate(x, duration, None, 16)[1]


@pytest.mark.parametrize("rnd", [False, True], ids=["soft", "round"])
@pytest.mark.parametrize("L", [1, 7, 300])
def test_items_kernel_equals_the_scalar_entry_and_the_regulators(L, rnd):
    pred, durs, pitch, energy = _items_inputs(L)
    distinct = torch.tensor(ROWS, device=DEV)
    for dk, use_p, use_e in itertools.product(durs, (False, True), (False, True)):
        dt, pt, et = durs[dk], pitch if use_p else None, energy if use_e else None
        tag = f"{dk} pitch={use_p} energy={use_e}"
        # equal rows: the bits of the scalar entry
        c = ROWS[1]
        want_d, want_f = runtime.infer_features(pred, dt, pt, et, *c, round_duration=rnd)
        dur, feats, frames = runtime.infer_features_items(pred, dt, pt, et, torch.tensor([c] * 3, device=DEV), round_duration=rnd)
        assert bits(dur) == bits(want_d) and bits(feats) == bits(want_f), tag
        assert torch.equal(frames, _regulated_len(dur, rnd)), tag
        # distinct rows: per item, the scalar entry on that item alone
        dur, feats, frames = runtime.infer_features_items(pred, dt, pt, et, distinct, round_duration=rnd)
        for b in range(3):
            sl = slice(b, b + 1)
            one_d, one_f = runtime.infer_features(pred[sl], None if dt is None else dt[sl], None if pt is None else pt[sl],
                                                  None if et is None else et[sl], *ROWS[b], round_duration=rnd)
            assert bits(dur[sl]) == bits(one_d) and bits(feats[sl]) == bits(one_f), (tag, b)
        reg = _regulated_len(dur, rnd)
        assert torch.equal(frames, reg), (tag, frames.tolist(), reg.tolist())
        assert np.array_equal(frames.cpu().numpy(), R.frames_wanted_ref(dur.cpu().numpy(), rnd)), tag
        # the float64 algebra (loose: the bits are pinned above)
        ref_d, ref_f = R.infer_features_items_ref(pred.cpu().numpy(), None if dt is None else dt.cpu().numpy(),
                                                  pt.cpu().numpy() if use_p else None, et.cpu().numpy() if use_e else None, ROWS, rnd)
        if not rnd:
            assert np.abs(dur.cpu().numpy() - ref_d).max() <= 1e-5 * max(1.0, np.abs(ref_d).max()), tag
        assert np.abs(feats.cpu().numpy() - ref_f).max() <= 1e-5 * max(1.0, np.abs(ref_f).max()), tag
        # without frames_wanted: no other bit changes
        d2, f2, none = runtime.infer_features_items(pred, dt, pt, et, distinct, round_duration=rnd, want_frames=False)
        assert none is None and bits(d2) == bits(dur) and bits(f2) == bits(feats), tag


@pytest.mark.parametrize("L", [1, 7, 300])
def test_frames_wanted_at_the_rounding_edge(L):
    """Durations (given as fp32 targets, which pass through) whose row sums land within 1e-3 of k + 0.5, and - hard mode -
    single durations within 1e-4 of k + 0.5: frames_wanted is what the regulators report."""
    g = np.random.default_rng(L)
    k = 10
    rows = []
    for delta in (-5e-4, 0.0, 5e-4):
        w = g.uniform(0.5, 1.5, L)
        rows.append((w * ((k + 0.5 + delta) / w.sum())).astype(np.float32))
    d = np.stack(rows)
    assert np.abs(d.astype(np.float64).sum(axis=1) - (k + 0.5)).max() < 1e-3
    pred = torch.zeros((3, L, 3), device=DEV)
    c = longform.make_controls(3, device=DEV)
    dur, _, frames = runtime.infer_features_items(pred, torch.from_numpy(d).to(DEV), None, None, c)
    assert bits(dur) == d.tobytes()
    reg = _regulated_len(dur, False)
    print(f"L={L}: soft sums {d.astype(np.float64).sum(axis=1)} -> frames_wanted {frames.tolist()}, regulator {reg.tolist()}")
    assert torch.equal(frames, reg) and np.array_equal(frames.cpu().numpy(), R.frames_wanted_ref(d))
    assert set(frames.tolist()) <= {k, k + 1}
    h = (g.integers(0, 5, (3, L)) + 0.5 + g.choice([-1e-4, 0.0, 1e-4], (3, L))).astype(np.float32)
    dur, _, frames = runtime.infer_features_items(pred, torch.from_numpy(h).to(DEV), None, None, c, round_duration=True)
    assert torch.equal(frames, _regulated_len(dur, True)) and np.array_equal(frames.cpu().numpy(), R.frames_wanted_ref(h, True))


# ------------------------------------------------------------------------------------------------ the model
def _model_inputs():
    inp = synth.make_inputs(2, 16, 192, variable=True, seed=33)
    return inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)


def _infer(model, controls=None, **scalars):
    text, tl, noise = _model_inputs()
    kw = {} if controls is None else {"controls": controls}
    mel, ao = model.infer(text, text_lengths=tl, steps=4, flow_noise=noise, max_dec_len=192, **scalars, **kw)
    fw = model.temporal_adaptor.frames_wanted if controls is not None else None
    torch.cuda.synchronize()
    return mel, ao, fw


SCALARS = [dict(duration_factor=1.1, pitch_factor=0.9, pitch_delta=0.2), dict(duration_factor=0.8, pitch_factor=1.15, pitch_delta=-0.4)]


def _row(s):
    return (s["duration_factor"], s["pitch_factor"], s["pitch_delta"], 1.0, 0.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_model_equal_control_rows_give_the_scalar_bits(gpu_model, dtype):
    try:
        gpu_model.set_compute_dtype(dtype)
        mel_s, ao_s, _ = _infer(gpu_model, **SCALARS[0])
        mel_c, ao_c, fw = _infer(gpu_model, torch.tensor([_row(SCALARS[0])] * 2, device=DEV))
    finally:
        gpu_model.set_compute_dtype(torch.float32)
    print(f"{dtype}: frames_wanted {fw.tolist()}, dec_lengths {ao_c.dec_lengths.tolist()}")
    assert int(fw.max()) <= 192                       # nothing is cut, so the clamp of the controls path does not act
    assert bits(mel_c) == bits(mel_s)
    for name in ("duration", "pitch", "energy", "dec_lengths"):
        assert bits(getattr(ao_c, name)) == bits(getattr(ao_s, name)), name
    assert torch.equal(fw, ao_c.dec_lengths)


def test_model_distinct_rows_equal_the_scalar_runs_per_item(gpu_model):
    mel_c, ao_c, fw = _infer(gpu_model, torch.tensor([_row(s) for s in SCALARS], device=DEV))
    assert int(fw.max()) <= 192
    for b, s in enumerate(SCALARS):
        mel_s, ao_s, _ = _infer(gpu_model, **s)
        for name in ("duration", "pitch", "energy", "dec_lengths"):
            assert bits(getattr(ao_c, name)[b]) == bits(getattr(ao_s, name)[b]), (b, name)
        n = int(ao_s.dec_lengths[b])
        err = float((mel_c[b, :, :n] - mel_s[b, :, :n]).abs().max())
        print(f"item {b}: dec_len {n}, mel L-inf against the scalar run {err:.3e}")
        assert n > 0 and err <= 1e-4


def test_model_reports_a_truncated_item(gpu_model):
    """duration_factor 3 on item 0 asks for more than the 192 frames of the capture: dec_lengths stays 192, frames_wanted tells.
    (The flow noise's duration channel is raised by 1, so that the 16 tokens ask for 142 frames at factor 1 - measured - and
    for 425 at factor 3.)"""
    text, tl, noise = _model_inputs()
    noise = noise.clone()
    noise[..., 0] += 1.0
    got = {}
    for f in (1.0, 3.0):
        _, ao = gpu_model.infer(text, text_lengths=tl, steps=4, flow_noise=noise, max_dec_len=192,
                                controls=longform.make_controls(2, duration_factor=[f, 1.0], device=DEV))
        got[f] = (gpu_model.temporal_adaptor.frames_wanted.tolist(), ao.dec_lengths.tolist())
        print(f"factor {f}: frames_wanted {got[f][0]}, dec_lengths {got[f][1]}")
    assert got[1.0][0] == got[1.0][1] and max(got[1.0][0]) <= 192
    fw, dl = got[3.0]
    assert fw[0] > 192 and dl[0] == 192
    assert fw[1] == dl[1] == got[1.0][0][1]                     # the other item is not touched


# ------------------------------------------------------------------------------------------------ the join
S_IN = TS + 8
BIG = 10 ** 6


def _join_case(tie=True):
    """Twelve items over three documents (document 1 empty), in reading order:
      doc 0: TS (pause -BIG: clamped to 1 by the 3-sample neighbour), 3 (-1), 257 (+100), 0 (0), 255 (-5: the last item, no overlap)
      doc 2: TS+1 (-BIG: clamped to (TS-1)/2), TS-1 (0), 256 (-100: clamped to 1), 2 (-1: clamped to 0), 1 (pause above every S_out)
    and two dropped items (doc -1 and doc 3).  The rows are given shuffled; pos is out of order and - with `tie` - has one tie,
    which the item index breaks."""
    reading = [(0, 5, TS, -BIG), (0, 7, 3, -1), (0, 7 if tie else 8, 257, 100), (0, 9, 0, 0), (0, 20, 255, -5),
               (2, -3, TS + 1, -BIG), (2, 0, TS - 1, 0), (2, 4, 256, -100), (2, 5, 2, -1), (2, 6, 1, 10 ** 7),
               (-1, 0, 300, 7), (3, 1, 200, -7)]
    perm = [7, 1, 10, 5, 2, 9, 0, 11, 4, 6, 3, 8]          # rows as given; the tied pair (1, 2) keeps its order
    g = np.random.default_rng(17)
    B = len(reading)
    audio = np.full((B, S_IN + 5), np.nan, np.float32)      # padded row stride, NaN past every length
    doc, pos, ln, pause = (np.zeros(B, np.int64) for _ in range(4))
    for row, r in enumerate(perm):
        doc[row], pos[row], ln[row], pause[row] = reading[r]
        audio[row, :ln[row]] = g.uniform(-1.0, 1.0, ln[row]).astype(np.float32)
    bounds = np.stack([g.integers(0, 40, B), ln - g.integers(0, 40, B)], axis=1).astype(np.int64)
    bounds[0] = (300, 200)                                  # start past the end: nothing left
    bounds[1] = (-4, ln[1] + 50)                            # start below 0, end past the length
    bounds[3] = (10, S_IN + 1000)                           # end past the length
    gain = g.uniform(0.25, 2.0, B).astype(np.float32)
    return dict(audio=audio, audio_len=ln, doc=doc, pos=pos, pause=pause, bounds=bounds, gain=gain)


def _run_join(c, S_out, fade=0, use_bounds=False, use_gain=False, D=3, audio=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    a = t(c["audio"] if audio is None else audio)[:, :S_IN]
    out = longform.join_outputs(D, S_out, a.shape[0], DEV)
    full = torch.full((D, S_out + 7), 777.0, device=DEV)                    # a sentinel behind every row
    out["audio"] = full[:, :S_out]
    r = longform.join(a, t(c["audio_len"]), t(c["doc"]), t(c["pos"]), t(c["pause"]), num_docs=D, out_samples=S_out,
                      bounds=t(c["bounds"]) if use_bounds else None, gain=t(c["gain"]) if use_gain else None, fade=fade, out=out)
    torch.cuda.synchronize()
    assert bool((full[:, S_out:] == 777.0).all()), "a column at or past S_out was written"
    return {k: v.cpu().numpy() for k, v in r.items() if k != "plan"}


# S_out: holds every item (the last pause is cut) | cuts inside an item of both documents | cuts inside document 2's overlap
S_OUTS = {"all": 2 * TS + 37, "mid_item": TS + 452, "in_overlap": TS - TS // 4}
worst = {"rel": 0.0}


@pytest.mark.parametrize("fade", [0, 4, 1000])
@pytest.mark.parametrize("cut", list(S_OUTS))
def test_join_against_the_reference(cut, fade):
    c, S_out = _join_case(), S_OUTS[cut]
    for use_bounds, use_gain in itertools.product((False, True), (False, True)):
        got = _run_join(c, S_out, fade, use_bounds, use_gain)
        ref, scale, p = R.join_ref(c["audio"][:, :S_IN], c["audio_len"], c["doc"], c["pos"], c["pause"], 3, S_out,
                                   c["bounds"] if use_bounds else None, c["gain"] if use_gain else None, fade)
        tag = f"{cut} fade={fade} bounds={use_bounds} gain={use_gain}"
        assert got["audio_len"].tolist() == p["doc_len"] and got["wanted_len"].tolist() == p["wanted"], tag
        assert got["item_offset"].tolist() == p["off"] and got["item_len"].tolist() == p["item_len"], tag
        assert not np.isnan(got["audio"]).any(), tag
        for d in range(3):
            err = np.abs(got["audio"][d].astype(np.float64) - ref[d]).max()
            if scale[d] > 0:
                worst["rel"] = max(worst["rel"], err / scale[d])
            assert err <= JOIN_BOUND * scale[d], (tag, d, err, scale[d])
        if not use_bounds:
            assert p["doc_len"][1] == 0 and p["ov"][list(c["audio_len"]).index(TS + 1)] == (TS - 1) // 2     # the clamp acted
            if cut == "all":
                assert p["doc_len"][0] == p["wanted"][0] == TS + 613 and p["wanted"][2] > S_out == p["doc_len"][2]
    print(f"{cut} fade={fade}: worst |out - ref| / max |g x| so far {worst['rel']:.3e}")


def test_join_many_short_items_under_one_tile():
    """60 items of 1 .. 7 samples in two documents: more items under one tile than the kernel visits one by one, so every
    sample searches its item - against the same reference, under the same bound."""
    g = np.random.default_rng(23)
    B, S = 60, 9
    ln = (np.arange(B) % 7 + 1).astype(np.int64)
    audio = np.full((B, S + 3), np.nan, np.float32)
    for b in range(B):
        audio[b, :ln[b]] = g.uniform(-1.0, 1.0, ln[b])
    c = dict(audio=audio, audio_len=ln, doc=(np.arange(B) % 2).astype(np.int64), pos=g.permutation(B).astype(np.int64),
             pause=g.choice([-2, -1, 0, 3], B).astype(np.int64), gain=g.uniform(0.5, 2.0, B).astype(np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)        # noqa: E731
    for S_out, fade in ((400, 0), (400, 2), (97, 2)):
        r = longform.join(t(audio)[:, :S], t(ln), t(c["doc"]), t(c["pos"]), t(c["pause"]), num_docs=2, out_samples=S_out,
                          gain=t(c["gain"]), fade=fade)
        torch.cuda.synchronize()
        ref, scale, p = R.join_ref(audio[:, :S], ln, c["doc"], c["pos"], c["pause"], 2, S_out, None, c["gain"], fade)
        assert r["audio_len"].tolist() == p["doc_len"] and r["wanted_len"].tolist() == p["wanted"]
        assert r["item_offset"].tolist() == p["off"] and r["item_len"].tolist() == p["item_len"]
        assert max(len(it) for it in p["items"]) == 30 and sum(v > 0 for v in p["ov"]) >= 10
        got = r["audio"].cpu().numpy().astype(np.float64)
        for d in range(2):
            assert np.abs(got[d] - ref[d]).max() <= JOIN_BOUND * scale[d], (S_out, fade, d)


def test_join_is_the_concatenation_when_nothing_blends():
    c = _join_case()
    c["pause"] = np.abs(c["pause"]) % 301
    for S_out in (3 * TS, TS + 452):
        got = _run_join(c, S_out)
        want = R.concat_ref(c["audio"][:, :S_IN], c["audio_len"], c["doc"], c["pos"], c["pause"], 3, S_out)
        assert (got["audio"] == want).all()


def test_join_bits_of_a_document_survive():
    c = _join_case(tie=False)
    kw = dict(S_out=2 * TS + 37, fade=4, use_bounds=True, use_gain=True)
    base = _run_join(c, **kw)
    B = len(c["doc"])
    # a permutation of the items
    perm = np.random.default_rng(3).permutation(B)
    moved = _run_join({k: v[perm] for k, v in c.items()}, **kw)
    assert moved["audio"].tobytes() == base["audio"].tobytes()
    assert np.array_equal(moved["item_offset"], base["item_offset"][perm])
    # the other documents removed from the call
    for d in (0, 2):
        keep = np.flatnonzero(c["doc"] == d)
        alone = _run_join({k: v[keep] for k, v in c.items()}, **kw)
        assert alone["audio"][d].tobytes() == base["audio"][d].tobytes() and not alone["audio"][2 - d].any()
        assert alone["audio_len"][d] == base["audio_len"][d]
    # NaN, 0 or 1e30 in the padding
    for fill in (0.0, 1e30):
        a = c["audio"].copy()
        for b in range(B):
            a[b, c["audio_len"][b]:] = fill
        assert _run_join(c, audio=a, **kw)["audio"].tobytes() == base["audio"].tobytes()
    # lengths out of range count as 0
    zero, wild = dict(c), dict(c)
    zero["audio_len"], wild["audio_len"] = c["audio_len"].copy(), c["audio_len"].copy()
    i, j = int(np.flatnonzero(c["audio_len"] == 257)[0]), int(np.flatnonzero(c["audio_len"] == 256)[0])
    zero["audio_len"][[i, j]] = 0
    wild["audio_len"][[i, j]] = (S_IN + 1, -3)
    z, w = _run_join(zero, **kw), _run_join(wild, **kw)
    assert all(z[k].tobytes() == w[k].tobytes() for k in z)
    # a second call
    assert all(_run_join(c, **kw)[k].tobytes() == base[k].tobytes() for k in base)


def _device_case(c):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in c.items()}


class _Spy(TorchDispatchMode):
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


def test_join_issues_no_aten_ops_and_replays():
    c = _device_case(_join_case())
    S_out = 2 * TS + 37
    a = c["audio"][:, :S_IN]
    out = longform.join_outputs(3, S_out, a.shape[0], DEV)

    def run():
        return longform.join(a, c["audio_len"], c["doc"], c["pos"], c["pause"], num_docs=3, out_samples=S_out, bounds=c["bounds"],
                             gain=c["gain"], fade=4, out=out)

    run()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items() if k != "plan"}
    spy = _Spy()
    with spy:
        run()
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    g = graph.GraphedCall(run)
    for k in eager:
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert bits(out[k]) == bits(eager[k]), k


# ------------------------------------------------------------------------------------------------ the Synthesizer
B_S, L_S, M_S, D_S = 4, 16, 128, 2


@pytest.fixture(scope="module")
def hifigan():
    from isp_tts_amd.hifigan import HifiGan
    cfg = synth.HIFIGAN_DIMS["v1"]
    return HifiGan.from_state_dict(synth.make_hifigan_state_dict(), cfg).to(DEV).eval()


def _eager_chain(model, voc, item_c, doc_c, S_out, fade, text, tl, doc, pos, pause, controls, noise):
    """The Synthesizer's stages from their public pieces, over fresh tensors."""
    with torch.no_grad():
        mel, ao = model.infer(text, text_lengths=tl, steps=4, flow_noise=noise, max_dec_len=M_S, controls=controls)
        frames_wanted = model.temporal_adaptor.frames_wanted
        audio, audio_len = voc(mel, ao.dec_lengths)
        bounds, _, _, gain = runtime.audio_measure(audio, audio_len, item_c.device_tables(DEV), item_c.sample_rate, item_c.trim_mode,
                                                   item_c.trim_threshold, item_c.pad_frames, 0, 0.0, item_c.peak_limit)
        j = longform.join(audio, audio_len, doc, pos, pause, num_docs=D_S, out_samples=S_out, bounds=bounds, gain=gain, fade=fade)
        r = doc_c(j["audio"], j["audio_len"])
        pcm = to_pcm16(r["audio"], r["audio_len"])
    torch.cuda.synchronize()
    return dict(pcm=pcm, audio_len=r["audio_len"], item_offset=j["item_offset"], frames_wanted=frames_wanted)


def test_synthesizer_equals_the_eager_chain(gpu_model, hifigan):
    S_out, fade = 3 * M_S * 256, 64
    item_c, doc_c = AudioConditioner(22050, target_lufs=None), AudioConditioner(22050)
    syn = longform.Synthesizer(gpu_model, hifigan, batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=S_out, steps=4,
                               item_conditioner=item_c, doc_conditioner=doc_c, fade=fade)
    inp = synth.make_inputs(B_S, L_S, M_S, variable=True, seed=44)
    text, tl, noise = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)          # noqa: E731
    calls = [dict(doc=i64([0, 1, 0, 1]), pos=i64([1, 0, 0, 1]), pause=i64([0, 2000, -300, 0]),
                  controls=longform.make_controls(B_S, duration_factor=[1.0, 0.8, 1.2, 1.0], pitch_delta=[0.0, 0.3, 0.0, -0.3], device=DEV)),
             dict(doc=i64([1, 1, 0, -1]), pos=i64([0, 1, 0, 0]), pause=i64([-500, 0, 4000, 0]),
                  controls=longform.make_controls(B_S, duration_factor=[0.9, 1.1, 1.0, 1.0], pitch_factor=[1.0, 1.1, 0.9, 1.0], device=DEV))]
    kept = []
    for kw in calls:
        r = syn(text, tl, flow_noise=noise, **kw)
        torch.cuda.synchronize()
        got = {k: r[k].clone() for k in ("pcm", "audio_len", "item_offset", "frames_wanted", "wanted_len", "dec_lengths")}
        assert r["truncated"].dtype == torch.bool and r["truncated"].shape == (B_S,)
        want = _eager_chain(gpu_model, hifigan, item_c, doc_c, S_out, fade, text, tl, noise=noise, **kw)
        for k in want:
            assert bits(got[k]) == bits(want[k]), k
        assert int(got["pcm"].abs().max()) > 100 and bool((got["audio_len"] > 0).all())
        kept.append(got)
    assert bits(kept[0]["pcm"]) != bits(kept[1]["pcm"]) and kept[1]["item_offset"][3] == -1
    spy = _Spy()
    with spy:
        syn._graph.replay()
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    with pytest.raises(ValueError, match="text"):
        syn(text[:, :8], tl, calls[0]["doc"], calls[0]["pos"])
    with pytest.raises(ValueError, match="doc"):
        syn(text, tl, calls[0]["doc"].int(), calls[0]["pos"])
    with pytest.raises(runtime.IspkError, match="GPU"):
        syn(text.cpu(), tl, calls[0]["doc"], calls[0]["pos"])


def test_synthesizer_with_hard_durations(state_dict, hifigan):
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config(soft_duration=False)).eval()
    model.load_state_dict(state_dict, strict=True)
    model = model.to(DEV).requires_grad_(False)
    S_out = 2 * M_S * 256
    syn = longform.Synthesizer(model, hifigan, batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=S_out)
    inp = synth.make_inputs(B_S, L_S, M_S, variable=True, seed=44)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)          # noqa: E731
    r = syn(inp["text"].to(DEV), inp["text_len"].to(DEV), i64([0, 0, 1, 1]), i64([0, 1, 0, 1]), flow_noise=inp["flow_x0"].to(DEV))
    torch.cuda.synchronize()
    fw, dl = r["frames_wanted"], r["dec_lengths"]
    assert torch.equal(dl, fw.clamp(max=M_S)) and torch.equal(r["truncated"], fw > M_S)
    assert torch.equal(r["audio_len"], torch.minimum(r["wanted_len"], torch.tensor(S_out, device=DEV)))
    assert torch.equal(r["item_len"], dl * 256) and int(r["pcm"].abs().max()) > 100
