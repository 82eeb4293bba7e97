"""Long-form synthesis without a GPU: the definition's invariants on the numpy reference, hand-written known answers,
make_controls, and the argument errors of the Python and C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import longform_reference as R
from isp_tts_amd import longform, runtime

E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4


def random_case(rng, allow_negative=True, with_bounds=True):
    B, D, S = int(rng.integers(1, 9)), int(rng.integers(1, 4)), int(rng.integers(1, 24))
    audio = rng.standard_normal((B, S)).astype(np.float32)
    audio_len = rng.integers(-1, S + 2, B)
    doc = rng.integers(-1, D + 1, B)
    pos = rng.integers(0, 4, B)
    pause = rng.integers(-12 if allow_negative else 0, 8, B)
    bounds = rng.integers(-2, S + 3, (B, 2)) if with_bounds and rng.random() < 0.5 else None
    fade = int(rng.integers(0, 6))
    S_out = int(rng.integers(1, 3 * S + 10))
    return dict(audio=audio, audio_len=audio_len, doc=doc, pos=pos, pause=pause, D=D, S_out=S_out, bounds=bounds, fade=fade)


def test_invariants_of_the_definition():
    """h + t <= n; no sample under more than two items; inside an overlap the two weights add up to 1."""
    rng = np.random.default_rng(5)
    overlaps = 0
    for _ in range(400):
        c = random_case(rng)
        S = c["audio"].shape[1]
        p = R.join_plan_ref(c["audio_len"], c["doc"], c["pos"], c["pause"], S, c["D"], 10 ** 6, c["bounds"], c["fade"])
        for d in range(c["D"]):
            total = p["wanted"][d] + S + 1
            cover, wsum = np.zeros(total, np.int64), np.zeros(total, np.float64)
            for b in p["items"][d]:
                n = p["n"][b]
                assert p["h"][b] + p["t"][b] <= n and 0 <= p["ov"][b] <= n // 2 and p["adv"][b] >= 0
                cover[p["off"][b]:p["off"][b] + n] += 1
                wsum[p["off"][b]:p["off"][b] + n] += R.weights_ref(n, p["h"][b], p["t"][b])
            assert cover.max(initial=0) <= 2
            two = cover == 2
            overlaps += int(two.sum())
            assert np.abs(wsum[two] - 1.0).max(initial=0.0) <= 2.0 ** -22       # two fp32 quotients that add up to 1 exactly
    assert overlaps > 50                      # the cases did exercise overlaps


def test_plain_concatenation_when_nothing_blends():
    """fade 0, every pause >= 0, no gain, no bounds: the join is the concatenation of the items and their silences, exactly."""
    rng = np.random.default_rng(6)
    for _ in range(300):
        c = random_case(rng, allow_negative=False, with_bounds=False)
        got, _, _ = R.join_ref(c["audio"], c["audio_len"], c["doc"], c["pos"], c["pause"], c["D"], c["S_out"])
        want = R.concat_ref(c["audio"], c["audio_len"], c["doc"], c["pos"], c["pause"], c["D"], c["S_out"])
        assert np.array_equal(got, want.astype(np.float64))


def test_known_answers_three_items():
    """One document: a (4 samples, pause 2), b (6 samples, overlap 2 with c), c (4 samples), fade 1.
    off = 0, 6, 10; wanted = 4 + 2 + (6 - 2) + 4 = 14.  Ramps: a h=1 t=1; b h=1 t=2; c h=2 t=1."""
    audio = np.zeros((3, 8), np.float32)
    audio[0, :4] = [1, 2, 3, 4]
    audio[1, :6] = [10, 20, 30, 40, 50, 60]
    audio[2, :4] = [100, 200, 300, 400]
    # given out of order: item 2 is a, item 0 is b, item 1 is c
    audio = audio[[1, 2, 0]]
    out, scale, p = R.join_ref(audio, [6, 4, 4], [0, 0, 0], [1, 2, 0], [-2, 0, 2], 1, 16, fade=1)
    assert p["order"] == [2, 0, 1] and p["off"] == [6, 10, 0] and p["ov"] == [2, 0, 0] and p["adv"] == [4, 4, 6]
    assert p["h"] == [1, 2, 1] and p["t"] == [2, 1, 1] and p["wanted"] == [14] and p["doc_len"] == [14]
    want = [0.5 * 1, 2, 3, 0.5 * 4, 0, 0,                               # a with its one-sample fades, then the pause
            0.5 * 10, 20, 30, 40,                                         # b: fade in, body
            0.75 * 50 + 0.25 * 100, 0.25 * 60 + 0.75 * 200,               # the crossfade: (3/4, 1/4), (1/4, 3/4)
            300, 0.5 * 400, 0, 0]                                         # c's body and fade out; silence past the document
    assert np.array_equal(out[0], np.array(want, np.float64)) and scale[0] == 400.0
    cut, _, pc = R.join_ref(audio, [6, 4, 4], [0, 0, 0], [1, 2, 0], [-2, 0, 2], 1, 11, fade=1)
    assert pc["doc_len"] == [11] and pc["wanted"] == [14] and np.array_equal(cut[0], out[0, :11])


def test_frames_wanted_reference_rounds_like_the_regulators():
    d = np.array([[0.25, 0.25, 0.999], [1.5, 2.5, 0.49]], np.float32)
    assert R.frames_wanted_ref(d).tolist() == [1, 4]                     # 1.499 -> 1; 4.49 -> 4
    assert R.frames_wanted_ref(d, round_duration=True).tolist() == [1, 5]  # (0, 0, 1); (2, 3, 0)


def test_control_algebra_reference():
    pred = np.array([[[np.log(3.0), 0.5, -1.0], [np.log(1.5), 2.0, 4.0]]])   # exp - 1 = 2, 0.5
    d, f = R.infer_features_items_ref(pred, None, None, None, [[2.0, 3.0, 1.0, 0.5, -1.0]])
    assert np.allclose(d, [[4.0, 1.0]]) and np.allclose(f, [[[2.5, -1.5], [7.0, 1.0]]])
    d, _ = R.infer_features_items_ref(pred, [[-1, 7]], None, None, [[1.2, 1, 0, 1, 0]], round_duration=True)
    assert d.tolist() == [[2.0, 7.0]]                                     # rint(2.4) = 2; the target where it is >= 0
    assert np.rint(2.5) == 2.0 and np.rint(3.5) == 4.0                    # (half to even, as the kernel's rintf)


def test_make_controls():
    c = longform.make_controls(3)
    assert c.dtype == torch.float32 and c.shape == (3, 5) and c.tolist() == [[1.0, 1.0, 0.0, 1.0, 0.0]] * 3
    c = longform.make_controls(3, duration_factor=[1.0, 0.5, 2.0], pitch_factor=1.5, pitch_delta=[10.0, 0.0, -5.0],
                               energy_factor=np.array([1.0, 2.0, 3.0]), energy_delta=torch.tensor(0.25), pitch_std=2.5)
    assert c.tolist() == [[1.0, 1.5, 4.0, 1.0, 0.25], [0.5, 1.5, 0.0, 2.0, 0.25], [2.0, 1.5, -2.0, 3.0, 0.25]]
    with pytest.raises(ValueError, match="pitch_factor"):
        longform.make_controls(3, pitch_factor=[1.0, 2.0])


def test_scalars_together_with_controls_are_refused():
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    text, c = torch.zeros((2, 4), dtype=torch.int64), longform.make_controls(2)
    for kw in (dict(duration_factor=1.5), dict(pitch_factor=0.9), dict(pitch_delta=3.0)):
        with pytest.raises(ValueError, match="controls"):
            model.infer(text, text_lengths=torch.tensor([4, 4]), controls=c, **kw)
    enc = torch.zeros((2, 4, 8))
    for kw in (dict(energy_factor=2.0), dict(energy_delta=0.5), dict(duration_factor=0.5)):
        with pytest.raises(ValueError, match="controls"):
            model.temporal_adaptor.infer(enc, controls=c, **kw)
    with pytest.raises(ValueError, match=r"fp32 \[2, 5\]"):
        model.temporal_adaptor.infer(enc, controls=c[:, :4])


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    one = ctypes.c_void_p(16)    # never dereferenced: the checks come before any launch
    items = lib.ispk_infer_features_items_f32      # (pred, dur_f32, dur_i64, pitch, energy, controls, round, dur, feats, frames, B, L, s)
    assert items(None, None, None, None, None, one, 0, one, one, None, 2, 4, None) == E_NULL
    assert b"null" in lib.ispk_last_error_string()
    assert items(one, None, None, None, None, None, 0, one, one, None, 2, 4, None) == E_NULL      # controls
    assert items(one, one, one, None, None, one, 1, one, one, one, 2, 4, None) == E_UNSUP
    assert b"one duration target" in lib.ispk_last_error_string()
    assert items(one, None, None, None, None, one, 0, one, one, one, 2, 0, None) == E_SHAPE
    assert items(one, None, None, None, None, one, 0, one, one, one, -1, 4, None) == E_SHAPE
    n = lib.ispk_join_plan_bytes()
    assert n == runtime.JOIN_PLAN_BYTES and lib.ispk_join_tile_samples() == runtime.JOIN_TILE_SAMPLES
    plan = lib.ispk_join_plan      # (audio_len, doc, pos, pause, bounds, plan, bytes, item_off, item_len, doc_len, wanted, B, S, D, S_out, fade, s)
    assert plan(None, one, one, None, None, one, n, one, one, one, one, 2, 8, 1, 8, 0, None) == E_NULL
    assert plan(one, one, one, None, None, None, n, one, one, one, one, 2, 8, 1, 8, 0, None) == E_NULL
    assert plan(one, one, one, None, None, one, n, one, one, one, one, 1025, 8, 1, 8, 0, None) == E_SHAPE
    assert b"1024" in lib.ispk_last_error_string()
    assert plan(one, one, one, None, None, one, n, one, one, one, one, 2, 8, 1025, 8, 0, None) == E_SHAPE
    assert plan(one, one, one, None, None, one, n, one, one, one, one, 2, 8, 0, 8, 0, None) == E_SHAPE
    assert plan(one, one, one, None, None, one, n, one, one, one, one, 2, 8, 1, 8, -1, None) == E_SHAPE
    assert b"fade" in lib.ispk_last_error_string()
    assert plan(one, one, one, None, None, one, n, one, one, one, one, 2, 8, 1, 8, 1 << 23, None) == E_SHAPE
    assert plan(one, one, one, None, None, one, n - 8, one, one, one, one, 2, 8, 1, 8, 0, None) == E_SHAPE
    assert plan(one, one, one, None, None, ctypes.c_void_p(8), n, one, one, one, one, 2, 8, 1, 8, 0, None) == E_ALIGN
    join = lib.ispk_join_f32       # (audio, ld_audio, gain, plan, doc_len, out, ld_out, B, S, D, S_out, s)
    assert join(None, 8, None, one, one, one, 8, 2, 8, 1, 8, None) == E_NULL
    assert join(one, 8, None, one, one, None, 8, 2, 8, 1, 8, None) == E_NULL
    assert join(one, 8, None, one, one, one, 8, 1025, 8, 1, 8, None) == E_SHAPE
    assert join(one, 8, None, one, one, one, 8, 2, 8, 1025, 8, None) == E_SHAPE
    assert join(one, 7, None, one, one, one, 8, 2, 8, 1, 8, None) == E_SHAPE
    assert join(one, 8, None, one, one, one, 7, 2, 8, 1, 8, None) == E_SHAPE
    assert b"strides" in lib.ispk_last_error_string()


def test_zero_sized_batches_are_noops():
    lib = runtime.lib()
    one = ctypes.c_void_p(16)
    assert lib.ispk_infer_features_items_f32(one, None, None, None, None, one, 0, one, one, one, 0, 4, None) == 0
    assert lib.ispk_join_plan(one, one, one, None, None, one, runtime.JOIN_PLAN_BYTES, one, one, one, one, 0, 8, 1, 8, 0, None) == 0
    assert lib.ispk_join_f32(one, 8, None, one, one, one, 8, 0, 8, 1, 8, None) == 0


def test_python_entries_refuse_cpu_tensors_and_bad_arguments():
    a, i64 = torch.zeros((2, 8)), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        longform.join(a, i64, i64, i64, num_docs=1, out_samples=8)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.infer_features_items(torch.zeros((2, 4, 3)), None, None, None, longform.make_controls(2))


def test_synthesizer_refuses_the_cpu():
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    from isp_tts_amd.hifigan import HifiGan
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    with pytest.raises(runtime.IspkError, match="GPU"):
        longform.Synthesizer(model, HifiGan(), batch=2, tokens=8, frames=32, docs=1, doc_samples=16384)
