"""Speech marks on the GPU (ispk_speech_marks, longform.speech_marks, Synthesizer(marks=True)) against the numpy reference
(tests/marks_reference.py).  The outputs are integers: every comparison is exact, there is no tolerance.  The reference counts
which clamps of the definition acted, and the tests assert that their cases reached each of them.  (Step 3's clamp can act in
the hard mode only: the soft mode's step 2 already stops at the length, which the reference counts as "len_cap".)"""
import numpy as np
import pytest
import torch

import marks_reference as M
from isp_tts_amd import graph, longform, runtime, synth
from isp_tts_amd.data import AudioConditioner
from test_gpu_longform import _Spy, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = 256


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def add_hits(total, h):
    for k, v in h.items():
        total[k] = total.get(k, 0) + int(v)


# ------------------------------------------------------------------------------------------------ shapes and modes
def _case(L, hard, seed=0):
    """B = 5 ragged items: text_len 0 and L among them; exact zeros, a NaN and a negative duration; lengths that fit, that cut
    the item, and that are out of range (those count as 0)."""
    g = np.random.default_rng(1000 * L + 10 * hard + seed)
    B = 5
    d = g.uniform(0.0, 3.0, (B, L)).astype(np.float32)
    d[g.random((B, L)) < 0.2] = 0.0
    if hard:
        d[1] = np.rint(d[1])
    text_len = np.array([L, 0, (L + 1) // 2, max(L - 1, 1), L], np.int64)
    if L >= 3:
        d[0, L // 2], d[4, L // 3] = np.nan, -2.5
    else:
        d[2, 0] = np.nan if hard else -1.0
    d[4, L - 1] = 2.0                                                      # item 4 (length out of range: 0) asks for samples
    frames = M.frames_from_sums(d, text_len, hard)
    S = int(HOP * (frames.max() + 2))
    audio_len = HOP * frames
    audio_len[3] = HOP * (frames[3] // 2)                                  # cut: the marks stop at the length
    audio_len[4] = S + 1                                                   # out of range: counts as 0
    pad = np.full((B, L + 3), 7.0, np.float32)                             # row stride L + 3
    pad[:, :L] = d
    return dict(d=d, dur=dev(pad)[:, :L], text_len=text_len, audio_len=audio_len, S=S, B=B)


def _synthetic_options(c, g, D=3):
    """Bounds, offsets, documents and document bounds that no join made: in range, out of range and crossing."""
    B, S = c["B"], c["S"]
    bounds = np.stack([g.integers(-5, S // 3 + 1, B), g.integers(S // 3, S + 6, B)], axis=1).astype(np.int64)
    bounds[2] = (S // 2, S // 4)                                           # start past the end: nothing is kept
    doc = np.array([0, 2, D, 1, 0], np.int64)                              # item 2: a document that does not exist
    off = g.integers(0, 2 * S + 1, B).astype(np.int64)
    off[3] = -1                                                            # item 3: dropped
    doc_len = g.integers(S // 2, 3 * S, D).astype(np.int64)
    doc_bounds = np.stack([g.integers(-5, S // 2, D), g.integers(S // 2, 3 * S + 6, D)], axis=1).astype(np.int64)
    # item 0 opens document 0, which is shorter than the item, begins before its bounds and ends after them
    off[0], doc_len[0], doc_bounds[0], doc_bounds[2] = 0, S // 2 + 3, (S // 8 + 1, S // 2), (-5, 10 * S)
    return bounds, off, doc, doc_len, doc_bounds


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 257, 4096])
def test_marks_equal_the_reference(L, hard):
    c = _case(L, hard)
    g = np.random.default_rng(L)
    B, S = c["B"], c["S"]
    assert c["dur"].stride(0) == L + 3
    bounds, off, doc, doc_len, doc_bounds = _synthetic_options(c, g)
    tl, al = dev(c["text_len"]), dev(c["audio_len"])
    hits = {}
    for W in (1, 7, 1024):
        word_id = g.integers(-1, W + 1, (B, L)).astype(np.int64)            # -1 and W: ignored
        word_id[:, L // 2:][word_id[:, L // 2:] == W // 2] = -1            # word W // 2 ends early; W = 1: tokens apart
        out = longform.marks_outputs(B, L, W, DEV)
        for opts in ({}, dict(bounds=bounds), dict(item_offset=off, doc=doc, doc_len=doc_len),
                     dict(bounds=bounds, item_offset=off, doc=doc, doc_len=doc_len, doc_bounds=doc_bounds)):
            for t in out.values():
                t.fill_(-77)
            runtime.speech_marks(c["dur"], tl, al, out["token_marks"], out["word_marks"], HOP, S, hard,
                                 **{k: dev(v) for k, v in opts.items()}, word_id=dev(word_id))
            tok, wrd, h = M.marks_ref(c["d"], c["text_len"], c["audio_len"], HOP, S, hard, word_id=word_id, W=W, **opts)
            add_hits(hits, h)
            tag = f"L={L} hard={hard} W={W} {sorted(opts)}"
            assert np.array_equal(host(out["token_marks"]), tok), tag
            assert np.array_equal(host(out["word_marks"]), wrd), tag
    # text_len None: every item has L tokens; no words: word_marks is not needed
    out = longform.marks_outputs(B, L, 0, DEV)
    runtime.speech_marks(c["dur"], None, al, out["token_marks"], None, HOP, S, hard)
    tok, _, _ = M.marks_ref(c["d"], None, c["audio_len"], HOP, S, hard)
    assert np.array_equal(host(out["token_marks"]), tok)
    print(f"L={L} hard={hard}: clamps taken by the reference {hits}")
    want = ["clamp3" if hard else "len_cap", "dropped", "word_ignored"]
    if L > 1:       # one token of about a frame and a half lies inside every bound
        want += ["clamp4", "clamp5", "clamp6", "bounds_fixed", "doc_bounds_fixed"]
    assert all(hits[k] > 0 for k in want), hits


def test_words_empty_apart_and_out_of_range():
    """One item of 6 tokens with hard durations 1 each at hop 10: word 0 = tokens 0 and 4 (not contiguous), word 1 has no
    token, word 2 = token 2; ids -1, 3 (= W) and 2^40 are ignored."""
    d = torch.ones((1, 6), device=DEV)
    word_id = torch.tensor([[0, -1, 2, 3, 0, 2 ** 40]], device=DEV)
    r = longform.speech_marks(d, None, torch.tensor([60], device=DEV), samples_per_frame=10, hard=True, word_id=word_id, words=3)
    assert r["token_marks"].tolist() == [[[10 * t, 10 * t + 10] for t in range(6)]]
    assert r["word_marks"].tolist() == [[[0, 50], [-1, -1], [20, 30]]]


# ------------------------------------------------------------------------------------------------ a real join
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_optional_inputs_with_a_real_join(hard):
    """Seven items of 12 tokens over three documents, joined by longform.join: negative pauses (crossfades), one dropped item,
    document 0 cut by out_samples; then a trimming AudioConditioner on the joined documents, whose first items begin with
    2,048 samples of near-silence.  All four sets of optional inputs against the reference, and the clamps they must reach."""
    g = np.random.default_rng(77 + hard)
    B, L, D, W = 7, 12, 3, 4
    d = g.uniform(0.5, 4.0, (B, L)).astype(np.float32)
    d[g.random((B, L)) < 0.15] = 0.0
    text_len = np.array([12, 12, 9, 12, 12, 1, 12], np.int64)
    frames = M.frames_from_sums(d, text_len, hard)
    cap = int(frames.max()) - 2                                            # the frame cap of a capture: the longest items are cut
    audio_len = HOP * np.minimum(frames, cap)
    S = HOP * cap
    audio = g.uniform(-0.5, 0.5, (B, S)).astype(np.float32)
    doc = np.array([0, 1, 0, 2, -1, 1, 0], np.int64)                       # item 4 is dropped
    pos = np.array([0, 0, 1, 0, 0, 1, 2], np.int64)
    pause = np.array([-300, -50, 500, 0, 0, 0, 0], np.int64)
    for first in (0, 1, 3):                                                # the first item of each document: a silent lead
        audio[first, :2048] *= 1e-5
        assert audio_len[first] >= 4096
    bounds = np.stack([g.integers(0, 200, B), audio_len - g.integers(0, 200, B)], axis=1).astype(np.int64)
    bounds[6] = (-9, audio_len[6] + 9)                                     # outside on both sides
    word_id = np.sort(g.integers(0, W + 1, (B, L)), axis=1).astype(np.int64)
    cond = AudioConditioner(22050, target_lufs=None)
    a, tl, al, dc, wid = dev(audio), dev(text_len), dev(audio_len), dev(doc), dev(word_id)
    hits = {}
    for use_bounds in (False, True):
        bd = bounds if use_bounds else None
        S_out = 3 * S                                                      # a first join to learn document 0's length
        j = longform.join(a, al, dc, dev(pos), dev(pause), num_docs=D, out_samples=S_out, bounds=None if bd is None else dev(bd), fade=16)
        wanted0 = int(j["wanted_len"][0])
        S_out = wanted0 - 700                                              # document 0 is cut inside its last item
        j = longform.join(a, al, dc, dev(pos), dev(pause), num_docs=D, out_samples=S_out, bounds=None if bd is None else dev(bd), fade=16)
        r = cond(j["audio"], j["audio_len"])
        torch.cuda.synchronize()
        off, doc_len, doc_bounds = host(j["item_offset"]), host(j["audio_len"]), host(r["bounds"])
        assert off[4] == -1 and int(j["wanted_len"][0]) > S_out == doc_len[0]
        assert (doc_bounds[:, 0] > 0).all() and (doc_bounds[:, 1] <= doc_len).all()      # the conditioner did trim
        assert off[2] < off[0] + (audio_len[0] if bd is None else bd[0, 1] - bd[0, 0])    # a crossfade: item 2 begins inside item 0
        for opts in (dict(bounds=bd), dict(bounds=bd, joined=j, doc=dc), dict(bounds=bd, joined=j, doc=dc, doc_bounds=r["bounds"])):
            got = longform.speech_marks(dev(d), tl, al, samples_per_frame=HOP, hard=hard, word_id=wid, words=W,
                                        **{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in opts.items()})
            ref_kw = dict(bounds=bd)
            if "joined" in opts:
                ref_kw.update(item_offset=off, doc=doc, doc_len=doc_len)
            if "doc_bounds" in opts:
                ref_kw.update(doc_bounds=doc_bounds)
            tok, wrd, h = M.marks_ref(d, text_len, audio_len, HOP, hard=hard, word_id=word_id, W=W, **ref_kw)
            add_hits(hits, h)
            tag = f"hard={hard} bounds={use_bounds} {sorted(opts)}"
            assert np.array_equal(host(got["token_marks"]), tok), tag
            assert np.array_equal(host(got["word_marks"]), wrd), tag
            if "joined" in opts and "doc_bounds" not in opts:
                # under the crossfade the marks of the two items overlap, as their audio does
                assert tok[2, 0, 0] == off[2] < tok[0, text_len[0] - 1, 1]
    print(f"hard={hard}: clamps taken by the reference {hits}")
    assert all(hits[k] > 0 for k in ("clamp3" if hard else "len_cap", "clamp4", "clamp5", "clamp6", "bounds_fixed", "dropped",
                                     "word_ignored")), hits


# ------------------------------------------------------------------------------------------------ determinism, no ATen op
def test_two_calls_and_a_replay_are_identical_and_issue_no_aten_op():
    c = _case(257, False)
    g = np.random.default_rng(5)
    bounds, off, doc, doc_len, doc_bounds = (dev(v) for v in _synthetic_options(c, g))
    tl, al, wid = dev(c["text_len"]), dev(c["audio_len"]), dev(g.integers(-1, 8, (c["B"], 257)))
    out = longform.marks_outputs(c["B"], 257, 7, DEV)

    def run():
        runtime.speech_marks(c["dur"], tl, al, out["token_marks"], out["word_marks"], HOP, c["S"], False, bounds, off, doc, doc_len,
                             doc_bounds, wid)

    run()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in out.items()}
    assert int(first["token_marks"].max()) > 0 and int(first["word_marks"].max()) > 0
    spy = _Spy()
    with spy:
        run()
        longform.speech_marks(c["dur"], tl, al, samples_per_frame=HOP, out=dict(token_marks=out["token_marks"], word_marks=None))
        run()
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert all(bits(out[k]) == bits(first[k]) for k in out)
    gr = graph.GraphedCall(run)
    for t in out.values():
        t.zero_()
    gr.replay()
    torch.cuda.synchronize()
    assert all(bits(out[k]) == bits(first[k]) for k in out)


def test_bad_shapes_are_refused():
    d, n = torch.zeros((2, 8), device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=DEV)      # noqa: E731
    for kw, match in ((dict(text_len=i64(3)), "text_len"), (dict(audio_len=n.int()), "audio_len"), (dict(bounds=i64(2, 3)), "bounds"),
                      (dict(word_id=i64(2, 7), words=2), "word_id"), (dict(out=dict(token_marks=i64(2, 7, 2), word_marks=None)), "token_marks"),
                      (dict(words=2, out=dict(token_marks=i64(2, 8, 2), word_marks=i64(2, 3, 2)[:, :2])), "word_marks")):
        with pytest.raises(ValueError, match=match):
            longform.speech_marks(d, kw.pop("text_len", n), kw.pop("audio_len", n), samples_per_frame=HOP, **kw)
    with pytest.raises(ValueError, match="doc_len"):
        runtime.speech_marks(d, n, n, i64(2, 8, 2), None, HOP, 8, False, None, n, n, None)


# ------------------------------------------------------------------------------------------------ forced alignment
def test_forced_alignment_marks_are_the_cumulative_durations():
    """A random monotone hard alignment (every frame belongs to one token, tokens in order) gives integer durations, as
    `attn_hard_dur` of a teacher-forced forward does; at hop 256 without a join the marks are 256 * cumsum, exactly."""
    g = np.random.default_rng(9)
    B, L = 3, 40
    text_len, mel_len = np.array([40, 23, 1], np.int64), np.array([300, 171, 64], np.int64)
    dur = np.zeros((B, L), np.int64)
    for b in range(B):
        token = np.sort(g.integers(0, text_len[b], mel_len[b]))             # frame -> token, monotone
        dur[b, :text_len[b]] = np.bincount(token, minlength=text_len[b])
    assert (dur.sum(axis=1) == mel_len).all() and (dur == 0).any()
    r = longform.speech_marks(dev(dur.astype(np.float32)), dev(text_len), dev(HOP * mel_len), samples_per_frame=HOP, hard=True)
    torch.cuda.synchronize()
    ends = HOP * np.cumsum(dur, axis=1)
    want = np.stack([ends - HOP * dur, ends], axis=2)
    want[np.arange(L)[None, :] >= text_len[:, None]] = -1
    assert np.array_equal(host(r["token_marks"]), want) and r["word_marks"].shape == (B, 0, 2)
    assert host(r["token_marks"])[np.arange(B), text_len - 1, 1].tolist() == (HOP * mel_len).tolist()


# ------------------------------------------------------------------------------------------------ the Synthesizer
B_S, L_S, M_S, D_S, W_S = 4, 16, 128, 2, 5
TODAY = {"pcm", "audio", "audio_len", "wanted_len", "item_offset", "item_len", "frames_wanted", "dec_lengths"}


@pytest.fixture(scope="module")
def hifigan():
    from isp_tts_amd.hifigan import HifiGan
    return HifiGan.from_state_dict(synth.make_hifigan_state_dict(), synth.HIFIGAN_DIMS["v1"]).to(DEV).eval()


def test_synthesizer_marks(gpu_model, hifigan):
    S_out = 30000                              # document 0 (items 2 and 0, 35,796 samples wanted) is cut
    syn = longform.Synthesizer(gpu_model, hifigan, batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=S_out, steps=4,
                               item_conditioner=AudioConditioner(22050, target_lufs=None), doc_conditioner=AudioConditioner(22050),
                               fade=64, marks=True, words=W_S)
    inp = synth.make_inputs(B_S, L_S, M_S, variable=True, seed=44)
    text, tl, noise = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV).clone()
    # Longer durations, as test_gpu_longform's truncation test raises them: at factor 3 item 0 asks for 28 frames (measured on the
    # MI355X; items 1 .. 3: 46, 13, 59), so at factor 20 it asks for about 188 and is cut at the 128 of the capture.
    noise[..., 0] += 1.0
    controls = longform.make_controls(B_S, duration_factor=[20.0, 1.0, 0.6, 1.0], device=DEV)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)          # noqa: E731
    doc, pos, pause = i64([0, 1, 0, -1]), i64([1, 0, 0, 0]), i64([0, 2000, -300, 0])
    word_id = (torch.arange(L_S, device=DEV) // 3).repeat(B_S, 1)          # three tokens a word; word 5 = W is ignored
    r = syn(text, tl, doc, pos, pause, controls, flow_noise=noise, word_id=word_id)
    torch.cuda.synchronize()
    assert set(r) == TODAY | {"token_marks", "word_marks", "duration", "item_audio_len", "item_bounds", "joined_len", "doc_bounds"}
    got = {k: r[k].clone() for k in r}
    # the marks are the reference's on the chain's own tensors
    np_ = {k: host(v) for k, v in got.items()}
    assert syn._hop == HOP
    tok, wrd, h = M.marks_ref(np_["duration"], host(tl), np_["item_audio_len"], HOP, M_S * HOP, False, np_["item_bounds"],
                              np_["item_offset"], host(doc), np_["joined_len"], np_["doc_bounds"], host(word_id), W_S)
    print(f"text_len {tl.tolist()}, frames_wanted {np_['frames_wanted'].tolist()}, item_audio_len {np_['item_audio_len'].tolist()}, "
          f"item_bounds {np_['item_bounds'].tolist()}, item_offset {np_['item_offset'].tolist()}, joined_len "
          f"{np_['joined_len'].tolist()}, doc_bounds {np_['doc_bounds'].tolist()}, clamps {h}")
    assert np.array_equal(np_["token_marks"], tok) and np.array_equal(np_["word_marks"], wrd)
    assert np.array_equal(M.frames_from_sums(np_["duration"], host(tl)), np_["frames_wanted"])
    assert bool(r["truncated"][0]) and np_["item_audio_len"][0] == M_S * HOP and h["len_cap"] > 0       # item 0 is cut at M frames
    assert np_["wanted_len"][0] > S_out == np_["joined_len"][0] and h["clamp5"] > 0                  # and document 0 at S_out
    assert h["dropped"] == 1 and (np_["token_marks"][3] == -1).all() and (np_["word_marks"][3] == -1).all()
    live = np_["token_marks"][0, :int(tl[0])]
    assert live.min() >= 0 and live.max() <= np_["audio_len"][0] and live[-1, 1] > live[0, 0]
    cues = longform.cues(r["word_marks"], doc, [[f"w{b}{w}" for w in range(W_S)] for b in range(B_S)], 22050)
    assert cues and all(c[0] in (0, 1) and c[1] <= c[2] for c in cues) and [c[0] for c in cues] == sorted(c[0] for c in cues)
    # a replay equals the eager chain over the same static buffers
    eager = syn._chain()
    torch.cuda.synchronize()
    for k in got:
        assert bits(eager[k]) == bits(got[k]), k
    # the replay issues no ATen op (and so no host read)
    spy = _Spy()
    with spy:
        syn._graph.replay()
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    # without word_id no token has a word
    r = syn(text, tl, doc, pos, pause, controls, flow_noise=noise)
    torch.cuda.synchronize()
    assert bool((r["word_marks"] == -1).all()) and bits(r["token_marks"]) == bits(got["token_marks"])
    with pytest.raises(ValueError, match="word_id"):
        syn(text, tl, doc, pos, word_id=word_id[:, :8])


def test_synthesizer_without_marks_is_todays(gpu_model, hifigan):
    syn = longform.Synthesizer(gpu_model, hifigan, batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=2 * M_S * HOP)
    assert set(syn.out) == TODAY and "word_id" not in syn.static and syn._marks is None
    with pytest.raises(ValueError, match="word_id"):
        syn(syn.static["text"], syn.static["text_len"], syn.static["doc"], syn.static["pos"],
            word_id=torch.zeros((B_S, L_S), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="words"):
        longform.Synthesizer(gpu_model, hifigan, batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=2 * M_S * HOP, words=3)
