"""Word-level prosody without a GPU: known answers of longform.prosody_spans, the numpy reference's own definition on a
hand-made case, and the argument errors of the Python and C entry points."""
import ctypes

import numpy as np
import pytest
import torch

import prosody_reference as P
from isp_tts_amd import longform, runtime

E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4
NEUTRAL = [1.0, 1.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------ prosody_spans
def test_spans_neutral_and_overlapping():
    c, g = longform.prosody_spans(2, 6, [])
    assert c.dtype == g.dtype == torch.float32 and c.shape == (2, 6, 5) and g.shape == (2, 6)
    assert c.tolist() == [[NEUTRAL] * 6] * 2 and g.tolist() == [[1.0] * 6] * 2
    # tokens 1 .. 3 and 3 .. 4 of item 1 overlap on token 3: factors multiply, deltas and decibels add, in the order given
    spans = [dict(item=1, tokens=(1, 4), duration_factor=2.0, pitch_delta=0.5, gain_db=-6.0),
             dict(item=1, tokens=(3, 5), duration_factor=1.5, pitch_factor=0.5, pitch_delta=0.25, energy_factor=3.0,
                  energy_delta=-1.0, gain_db=-14.0)]
    c, g = longform.prosody_spans(2, 6, spans)
    assert c[0].tolist() == [NEUTRAL] * 6 and g[0].tolist() == [1.0] * 6
    assert c[1].tolist() == [NEUTRAL, [2.0, 1.0, 0.5, 1.0, 0.0], [2.0, 1.0, 0.5, 1.0, 0.0], [3.0, 0.5, 0.75, 3.0, -1.0],
                             [1.5, 0.5, 0.25, 3.0, -1.0], NEUTRAL]
    want = np.array([1.0, 10 ** -0.3, 10 ** -0.3, 0.1, 10 ** -0.7, 1.0]).astype(np.float32)
    assert g[1].numpy().tobytes() == want.tobytes()                        # float64 on the host, one cast at the end


def test_spans_by_words_pitch_std_and_base():
    L = 9
    word_id = (torch.arange(L) // 3).repeat(2, 1)                          # three tokens a word
    word_id[1, 8] = -1                                                     # punctuation: belongs to no word
    base = longform.make_controls(2, duration_factor=[0.9, 1.25], energy_delta=[0.0, 0.5])
    c, g = longform.prosody_spans(2, L, [dict(item=0, words=(1, 2), pitch_delta=5.0, gain_db=20.0),
                                         dict(item=1, words=(1, 3), duration_factor=2.0)],
                                  base=base, word_id=word_id, pitch_std=2.5)
    b0, b1 = [np.float32(0.9).item(), 1.0, 0.0, 1.0, 0.0], [1.25, 1.0, 0.0, 1.0, 0.5]
    assert c[0].tolist() == [b0] * 3 + [[b0[0], 1.0, 2.0, 1.0, 0.0]] * 3 + [b0] * 3      # 5.0 / pitch_std; the base rows stay
    assert g[0].tolist() == [1.0] * 3 + [10.0] * 3 + [1.0] * 3
    assert c[1].tolist() == [b1] * 3 + [[2.5, 1.0, 0.0, 1.0, 0.5]] * 5 + [b1]            # word 2 without its last token
    assert g[1].tolist() == [1.0] * L
    # an empty range selects nothing
    c2, _ = longform.prosody_spans(2, L, [dict(item=0, tokens=(4, 4), duration_factor=9.0)], base=base)
    assert c2.tolist() == base[:, None, :].repeat(1, L, 1).tolist()


@pytest.mark.parametrize("span, key", [
    (dict(item=0, tokens=(0, 2), speed=2.0), "speed"),
    (dict(item=2, tokens=(0, 2)), "item"),
    (dict(item=-1, tokens=(0, 2)), "item"),
    (dict(tokens=(0, 2)), "item"),
    (dict(item=0, tokens=(0, 7)), "tokens"),
    (dict(item=0, tokens=(3, 2)), "tokens"),
    (dict(item=0, tokens=(-1, 2)), "tokens"),
    (dict(item=0, words=(2, 1)), "words"),
    (dict(item=0, tokens=(0, 2), words=(0, 1)), "tokens"),
    (dict(item=0, gain_db=3.0), "tokens"),
])
def test_spans_errors_name_the_key(span, key):
    with pytest.raises(ValueError, match=key):
        longform.prosody_spans(2, 6, [span], word_id=torch.zeros((2, 6), dtype=torch.int64))


def test_spans_words_need_word_id():
    with pytest.raises(ValueError, match="word_id"):
        longform.prosody_spans(2, 6, [dict(item=0, words=(0, 1), gain_db=-6.0)])
    with pytest.raises(ValueError, match="word_id"):
        longform.prosody_spans(2, 6, [], word_id=torch.zeros((2, 5), dtype=torch.int64))
    with pytest.raises(ValueError, match="base"):
        longform.prosody_spans(2, 6, [], base=longform.make_controls(3))


# ------------------------------------------------------------------------------------------------ the reference's definition
def test_reference_envelope_known_answer():
    """Two live tokens of 8 and 4 samples around a zero-length one, a dead one behind, ramp 3: h = min(3, 4, 2) = 2, the ramp
    covers samples 6 .. 9 with w = 1/8, 3/8, 5/8, 7/8; the tail behind E = 12 takes the last gain."""
    marks = [(0, 8), (8, 8), (8, 12), (-1, -1)]
    e, st = P.envelope_ref(14, marks, [1.0, 7.0, 3.0, 9.0], 3)
    assert e.tolist() == [1.0] * 6 + [1.25, 1.75, 2.25, 2.75] + [3.0] * 4
    assert st == dict(ramp=4, cut=4, steps=0, live=2, tail=2)
    e, st = P.envelope_ref(14, marks, [1.0, 7.0, 3.0, 9.0], 0)
    assert e.tolist() == [1.0] * 8 + [3.0] * 6 and st["steps"] == 1
    # a length inside the second token cuts it to 2 samples: h = 1
    e, _ = P.envelope_ref(10, marks, [1.0, 7.0, 3.0, 9.0], 3)
    assert e.tolist() == [1.0] * 7 + [1.5, 2.5, 3.0]
    assert P.envelope_ref(5, [(-1, -1)] * 3, [2.0] * 3, 3)[0].tolist() == [1.0] * 5
    out, _ = P.gain_envelope_ref(np.ones((2, 6)), [7, 3], np.array([[(0, 6)], [(0, 2)]]), [[2.0], [0.5]], 1)
    assert out.tolist() == [[0.0] * 6, [0.5, 0.5, 0.5, 0.0, 0.0, 0.0]]     # a length out of range counts as 0; the tail's gain


# ------------------------------------------------------------------------------------------------ the C entries
def test_argument_errors_without_gpu():
    lib = runtime.lib()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)    # never dereferenced: the checks come before any launch
    tokens = lib.ispk_infer_features_tokens_f32    # (pred, dur_f32, dur_i64, pitch, energy, controls, round, dur, feats, frames, B, L, s)
    assert tokens(None, None, None, None, None, one, 0, one, one, None, 2, 4, None) == E_NULL
    assert b"null" in lib.ispk_last_error_string()
    assert tokens(one, None, None, None, None, None, 0, one, one, None, 2, 4, None) == E_NULL     # controls
    assert tokens(one, None, None, None, None, one, 0, None, one, None, 2, 4, None) == E_NULL
    assert tokens(one, None, None, None, None, one, 0, one, None, None, 2, 4, None) == E_NULL
    assert tokens(one, one, one, None, None, one, 1, one, one, one, 2, 4, None) == E_UNSUP
    assert b"one duration target" in lib.ispk_last_error_string()
    assert tokens(one, None, None, None, None, one, 0, one, one, one, 2, 0, None) == E_SHAPE
    assert tokens(one, None, None, None, None, one, 0, one, one, one, -1, 4, None) == E_SHAPE
    assert lib.ispk_gain_envelope_tile_samples() == runtime.GAIN_TILE_SAMPLES
    env = lib.ispk_gain_envelope_f32               # (audio, ld_audio, audio_len, token_marks, token_gain, ramp, out, ld_out, B, L, S, s)
    for k in (0, 2, 3, 4, 6):
        args = [one, 8, one, one, one, 4, two, 8, 2, 4, 8, None]
        args[k] = None
        assert env(*args) == E_NULL, k
    assert b"null" in lib.ispk_last_error_string()
    assert env(one, 8, one, one, one, 4, two, 8, 2, 0, 8, None) == E_SHAPE                  # L
    assert env(one, 8, one, one, one, 4, two, 8, 2, 4097, 8, None) == E_SHAPE
    assert b"4096" in lib.ispk_last_error_string()
    assert env(one, 8, one, one, one, 4, two, 8, 65536, 4, 8, None) == E_SHAPE              # B
    assert env(one, 8, one, one, one, 4, two, 8, 2, 4, -1, None) == E_SHAPE                 # S
    assert env(one, 7, one, one, one, 4, two, 8, 2, 4, 8, None) == E_SHAPE                  # ld_audio < S
    assert env(one, 8, one, one, one, 4, two, 7, 2, 4, 8, None) == E_SHAPE                  # ld_out < S
    assert b"strides" in lib.ispk_last_error_string()
    assert env(one, 8, one, one, one, -1, two, 8, 2, 4, 8, None) == E_SHAPE                 # ramp
    assert env(one, 8, one, one, one, 1 << 22, two, 8, 2, 4, 8, None) == E_SHAPE
    assert b"ramp" in lib.ispk_last_error_string()
    # out overlaps audio without being audio: shifted by one sample, by one row, or the same base at another stride
    assert env(one, 8, one, one, one, 4, ctypes.c_void_p(20), 8, 2, 4, 8, None) == E_SHAPE
    assert b"overlaps" in lib.ispk_last_error_string()
    assert env(one, 8, one, one, one, 4, ctypes.c_void_p(16 + 32), 8, 2, 4, 8, None) == E_SHAPE
    assert env(one, 8, one, one, one, 4, one, 12, 2, 4, 8, None) == E_SHAPE


def test_zero_sized_batches_are_noops():
    lib = runtime.lib()
    one = ctypes.c_void_p(16)
    assert lib.ispk_infer_features_tokens_f32(one, None, None, None, None, one, 0, one, one, one, 0, 4, None) == 0
    assert lib.ispk_gain_envelope_f32(one, 8, one, one, one, 4, ctypes.c_void_p(1 << 20), 8, 0, 4, 8, None) == 0
    assert lib.ispk_gain_envelope_f32(one, 8, one, one, one, 4, one, 8, 0, 4, 8, None) == 0      # in place


# ------------------------------------------------------------------------------------------------ the Python entries
def test_three_dimensional_controls_are_checked_before_any_launch():
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    enc = torch.zeros((2, 4, 8))
    for bad in (torch.zeros((2, 4, 4)), torch.zeros((2, 4, 5), dtype=torch.float64), torch.zeros((2, 3, 5))):
        with pytest.raises(ValueError, match=r"fp32 \[2, 4, 5\]"):
            model.temporal_adaptor.infer(enc, controls=bad)
        with pytest.raises(ValueError, match=r"fp32 \[2, 4, 5\]"):
            model.infer(torch.zeros((2, 4), dtype=torch.int64), text_lengths=torch.tensor([4, 4]), controls=bad)
    with pytest.raises(ValueError, match="controls"):                      # the scalars stay at their defaults
        model.temporal_adaptor.infer(enc, controls=torch.ones((2, 4, 5)), energy_factor=2.0)
    with pytest.raises(ValueError, match=r"fp32 \[2, 5\]"):                # a 2-D tensor goes where it went
        model.temporal_adaptor.infer(enc, controls=torch.zeros((2, 4)))


def test_python_entries_refuse_cpu_tensors_and_bad_arguments():
    a, n = torch.zeros((2, 8)), torch.zeros(2, dtype=torch.int64)
    marks, gain = torch.zeros((2, 4, 2), dtype=torch.int64), torch.ones((2, 4))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        longform.gain_envelope(a, n, marks, gain)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.gain_envelope(a, n, marks, gain, 128, torch.empty_like(a))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.infer_features_tokens(torch.zeros((2, 4, 3)), None, None, None, torch.ones((2, 4, 5)))
    assert "infer_features_tokens" in runtime.__dict__ and "gain_envelope" in runtime.__dict__
    from isp_tts_amd.bindings import adaptor, audio
    assert "infer_features_tokens" in adaptor.__all__ and "gain_envelope" in audio.__all__
