"""Speech marks without a GPU: the definition's invariants on the numpy reference (tests/marks_reference.py), hand-written known
answers, the reference's frame counts against longform_reference.frames_wanted_ref, the argument errors of the C and Python
entry points, and the host helpers `cues` / `webvtt`."""
import ctypes

import numpy as np
import pytest
import torch

import longform_reference as R
import marks_reference as M
from isp_tts_amd import longform, runtime

E_NULL, E_SHAPE = -1, -2


def random_item_case(rng, hard):
    B, L, hop = int(rng.integers(1, 6)), int(rng.integers(1, 12)), int(rng.choice([2, 64, 256]))
    d = rng.uniform(0.0, 4.0, (B, L)).astype(np.float32)
    d[rng.random((B, L)) < 0.25] = 0.0                                     # exact zeros
    if hard:
        d = np.rint(d).astype(np.float32) if rng.random() < 0.5 else d
    text_len = rng.integers(0, L + 1, B)
    frames = M.frames_from_sums(d, text_len, hard)
    cap = int(rng.integers(1, 3 * L + 2))                                  # the capture's frame cap: some items are cut
    audio_len = hop * np.minimum(frames, cap)
    return dict(d=d, text_len=text_len, audio_len=audio_len, hop=hop, frames=frames, cap=cap)


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_invariants_of_the_definition(hard):
    """Starts <= ends, consecutive tokens tile, the first start is 0, the last end lies within hop / 2 of audio_len (exactly
    on it with hard durations) when the item is not cut, and on it when it is."""
    rng = np.random.default_rng(41 + hard)
    cut = empty = 0
    for _ in range(300):
        c = random_item_case(rng, hard)
        tok, _, _ = M.marks_ref(c["d"], c["text_len"], c["audio_len"], c["hop"], hard=hard)
        for b, n in enumerate(c["text_len"]):
            assert (tok[b, n:] == -1).all()
            if n == 0:
                empty += 1
                continue
            t = tok[b, :n]
            assert (t[:, 0] <= t[:, 1]).all() and (t[1:, 0] == t[:-1, 1]).all() and t[0, 0] == 0
            assert 0 <= t[-1, 1] <= c["audio_len"][b]
            if c["frames"][b] > c["cap"]:
                cut += 1
                assert t[-1, 1] == c["audio_len"][b]
            else:
                assert abs(int(t[-1, 1]) - int(c["audio_len"][b])) <= (0 if hard else c["hop"] // 2)
    assert cut > 20 and empty > 20


def test_invariants_through_bounds_and_a_join():
    """The clamps of steps 4 .. 6 keep the order: starts <= ends and tiling survive any bounds, offset and document length."""
    rng = np.random.default_rng(43)
    hits = {}
    for _ in range(300):
        c = random_item_case(rng, False)
        B, D = len(c["text_len"]), 2
        S = int(c["audio_len"].max()) + 3
        bounds = rng.integers(-3, S + 3, (B, 2))
        doc = rng.integers(-1, D + 1, B)
        off = np.where((doc >= 0) & (doc < D), rng.integers(0, 2 * S, B), -1)
        doc_len = rng.integers(0, 3 * S, D)
        doc_bounds = rng.integers(-3, 3 * S, (D, 2))
        tok, _, h = M.marks_ref(c["d"], c["text_len"], c["audio_len"], c["hop"], S, False, bounds, off, doc, doc_len, doc_bounds)
        for k, v in h.items():
            hits[k] = hits.get(k, 0) + v
        for b, n in enumerate(c["text_len"]):
            t = tok[b, :n]
            if off[b] < 0:
                assert (tok[b] == -1).all()
            elif n:
                assert (t[:, 0] <= t[:, 1]).all() and (t[1:, 0] == t[:-1, 1]).all() and t.min() >= 0
                assert t.max() <= doc_len[doc[b]]
    assert all(hits[k] > 0 for k in ("clamp4", "clamp5", "clamp6", "bounds_fixed", "doc_bounds_fixed", "dropped")), hits


def test_known_answers():
    """hop 256, the pair of rows test_longform_host uses for frames_wanted (1 and 4 frames soft, 1 and 5 hard).
    Soft, row 0 (len 256): s = 0, .25, .5, 1.499 -> v = .5, 64.5, 128.5, 384.2; the last is >= len + 1 -> 0, 64, 128, 256.
    Soft, row 1 (len 1024): s = 0, 1.5, 4, 4.49 -> v = .5, 384.5, 1024.5 (< 1025: floor), 1149.9 (>= 1025) -> 0, 384, 1024, 1024.
    Hard, row 0 (len 256): repeats 0, 0, 1 -> C = 0, 0, 0, 1 -> 0, 0, 0, 256.  Row 1 (len 1280): repeats 2, 3, 0 -> 0, 512, 1280, 1280.
    Words (0, 0, 1) on row 0 and (1, 7, 1) on row 1 with W = 2: word 1 of row 1 spans its two outer tokens, 7 is ignored."""
    d = np.array([[0.25, 0.25, 0.999], [1.5, 2.5, 0.49]], np.float32)
    words = [[0, 0, 1], [1, 7, 1]]
    tok, wrd, _ = M.marks_ref(d, [3, 3], [256, 1024], 256, word_id=words, W=2)
    assert tok.tolist() == [[[0, 64], [64, 128], [128, 256]], [[0, 384], [384, 1024], [1024, 1024]]]
    assert wrd.tolist() == [[[0, 128], [128, 256]], [[-1, -1], [0, 1024]]]
    tok, wrd, _ = M.marks_ref(d, [3, 3], [256, 1280], 256, hard=True, word_id=words, W=2)
    assert tok.tolist() == [[[0, 0], [0, 0], [0, 256]], [[0, 512], [512, 1280], [1280, 1280]]]
    assert wrd.tolist() == [[[0, 0], [0, 256]], [[-1, -1], [0, 1280]]]
    # item 1 trimmed to [100, 900), joined at offset 5000 into a document of 5600 samples, the document trimmed to [4000, 5500)
    tok, _, h = M.marks_ref(d, [3, 2], [256, 1024], 256, bounds=[[0, 256], [100, 900]], item_offset=[-1, 5000], doc=[0, 0],
                            doc_len=[5600], doc_bounds=[[4000, 5500]])
    # 0, 384, 1024 -> in [100, 900]: 0, 284, 800 -> + 5000, at most 5600: 5000, 5284, 5600 -> in [4000, 5500] - 4000
    assert tok.tolist() == [[[-1, -1]] * 3, [[1000, 1284], [1284, 1500], [-1, -1]]]
    assert h["dropped"] == 1 and h["clamp4"] == 2 and h["clamp5"] == 1 and h["clamp6"] == 1


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_frame_counts_are_the_regulators(hard):
    d = np.array([[0.25, 0.25, 0.999], [1.5, 2.5, 0.49]], np.float32)
    assert M.frames_from_sums(d, None, hard).tolist() == R.frames_wanted_ref(d, hard).tolist() == ([1, 5] if hard else [1, 4])
    rng = np.random.default_rng(7)
    for _ in range(50):
        d = rng.uniform(0.0, 6.0, (4, int(rng.integers(1, 40)))).astype(np.float32)
        d[rng.random(d.shape) < 0.2] = 0.0
        assert np.array_equal(M.frames_from_sums(d, None, hard), R.frames_wanted_ref(d, hard))


def test_argument_errors_without_gpu():
    marks = runtime.lib().ispk_speech_marks
    one = ctypes.c_void_p(16)    # never dereferenced: the checks come before any launch
    err = runtime.lib().ispk_last_error_string
    # (duration, ld, text_len, audio_len, bounds, item_offset, doc, doc_len, doc_bounds, word_id, token_marks, word_marks,
    #  hop, round, B, L, S, D, W, stream)
    ok = dict(duration=one, ld=8, text_len=None, audio_len=one, bounds=None, item_offset=None, doc=None, doc_len=None,
              doc_bounds=None, word_id=None, token_marks=one, word_marks=None, hop=256, round=0, B=2, L=8, S=4096, D=0, W=0)

    def call(**kw):
        return marks(*{**ok, **kw}.values(), None)

    for name in ("duration", "audio_len", "token_marks"):
        assert call(**{name: None}) == E_NULL, name
    assert b"null" in err()
    for part in ({"item_offset": one}, {"doc": one, "doc_len": one}, {"item_offset": one, "doc": one}):
        assert call(D=1, **part) == E_NULL, part
    assert b"together" in err()
    assert call(doc_bounds=one) == E_NULL and b"doc_bounds" in err()
    assert call(word_id=one, W=4) == E_NULL and call(W=4) == E_NULL
    join = dict(item_offset=one, doc=one, doc_len=one)
    for bad in (dict(L=4097), dict(W=1025, word_marks=one), dict(W=-1), dict(B=65536), dict(B=-1), dict(hop=0), dict(hop=(1 << 20) + 1),
                dict(S=-1), dict(ld=7), dict(D=0, **join), dict(D=1025, **join)):
        assert call(**bad) == E_SHAPE, bad
    assert b"1024" in err()
    assert call(L=4096, ld=4096, B=0) == 0 and call(L=0) == 0 and call(B=0, W=1024, word_marks=one, hop=1 << 20, **join, D=1024) == 0
    assert call(W=0, word_id=one, B=0) == 0      # word_marks may be NULL when W == 0
    assert runtime.MARKS_MAX_TOKENS == 4096 and runtime.MARKS_MAX_WORDS == 1024


def test_python_entries_refuse_cpu_tensors_and_bad_arguments():
    d, n = torch.zeros((2, 8)), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        longform.speech_marks(d, n, n, samples_per_frame=256)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.speech_marks(d, n, n, torch.zeros((2, 8, 2), dtype=torch.int64), None, 256, 4096)
    # what needs no device is checked first: the scalars, the pairing of the optional inputs and the duration's layout
    for kw, match in ((dict(samples_per_frame=0), "samples_per_frame"), (dict(samples_per_frame=2.5), "samples_per_frame"),
                      (dict(samples_per_frame=256, words=1025), "words"), (dict(samples_per_frame=256, doc=n), "go together"),
                      (dict(samples_per_frame=256, joined={"item_offset": n, "audio_len": n}), "go together"),
                      (dict(samples_per_frame=256, doc_bounds=n), "doc_bounds"),
                      (dict(samples_per_frame=256, word_id=torch.zeros((2, 8), dtype=torch.int64)), "words >= 1")):
        with pytest.raises(ValueError, match=match):
            longform.speech_marks(d, n, n, **kw)
    for bad in (torch.zeros((2, 8), dtype=torch.float64), torch.zeros((2, 8, 1)), torch.zeros((8, 2)).t(), torch.zeros((1, 4097))):
        with pytest.raises(ValueError, match="duration|L=4097"):
            longform.speech_marks(bad, n, n, samples_per_frame=256)
    out = longform.marks_outputs(3, 5, 2, "cpu")
    assert out["token_marks"].shape == (3, 5, 2) and out["word_marks"].shape == (3, 2, 2) and out["word_marks"].dtype == torch.int64


def test_cues_and_webvtt():
    """Two documents at 1 kHz.  Item 0 (doc 1): "b" 0 .. 500, "c" 500 .. 1250.  Item 1 (doc 0): "a" 100 .. 3723004, word 1 absent.
    Item 2: dropped (all -1).  Item 3 (doc 1), given after item 0 but earlier in the document: "<d&>" 0 .. 250."""
    wm = torch.tensor([[[0, 500], [500, 1250]], [[100, 3723004], [-1, -1]], [[-1, -1], [-1, -1]], [[0, 250], [-1, -1]]])
    doc = torch.tensor([1, 0, -1, 1])
    labels = [["b", "c"], ["a", "unused"], ["x", "y"], ["<d&>"]]
    got = longform.cues(wm, doc, labels, 1000)
    assert got == [(0, 0.1, 3723.004, "a"), (1, 0.0, 0.25, "<d&>"), (1, 0.0, 0.5, "b"), (1, 0.5, 1.25, "c")]
    assert longform.webvtt(got[:1]) == "WEBVTT\n\n1\n00:00:00.100 --> 01:02:03.004\na\n"
    assert longform.webvtt(got[1:]) == ("WEBVTT\n\n1\n00:00:00.000 --> 00:00:00.250\n&lt;d&amp;&gt;\n\n"
                                       "2\n00:00:00.000 --> 00:00:00.500\nb\n\n3\n00:00:00.500 --> 00:00:01.250\nc\n")
    assert longform.webvtt([]) == "WEBVTT\n"
    with pytest.raises(ValueError, match="one document"):
        longform.webvtt(got)
    with pytest.raises(ValueError, match="labels"):
        longform.cues(wm, doc, labels[:2], 1000)
