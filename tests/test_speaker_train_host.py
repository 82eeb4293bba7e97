"""CPU: the host side of multi-speaker training - the `speaker_in_forward` switch, `extend_speakers`, the optional `speaker` field
of `ingest.BatchIngest`, and the fixture tests/golden/speaker_train.npz (tools/make_speaker_train_goldens.py).  The kernels and the
model on the GPU: tests/test_gpu_speaker_train.py."""
import numpy as np
import pytest
import torch

from conftest import crc, golden

import hard_duration_reference as hdr
from isp_tts_amd import ingest, synth
from isp_tts_amd.acoustic import AcousticModel
from isp_tts_amd.config import AcousticDims


def _multi(**kw):
    return AcousticModel.init(dict(AcousticDims().model_config(), num_speakers=4), **kw).eval()


def _call(model, **kw):
    inp = synth.make_inputs(1, 16, 32)
    return model(inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"], inp["energy"], **kw)


def test_the_switch_is_off_by_default_and_stays_out_of_the_state_dict():
    off, on = _multi(), _multi(speaker_in_forward=True)
    assert off.speaker_in_forward is False and on.speaker_in_forward is True
    assert AcousticModel.init(AcousticDims().model_config()).speaker_in_forward is False
    assert list(off.state_dict()) == list(on.state_dict())
    with pytest.raises(AttributeError, match="speaker_encoder"):                 # off: the reference's own error
        _call(off, speaker=torch.zeros(1, 1, dtype=torch.long))
    off.speaker_in_forward = True                                                # a plain attribute: may be set after loading
    assert list(off.state_dict()) == list(on.state_dict())
    with pytest.raises(ValueError, match="speaker"):
        _call(off)
    with pytest.raises(ValueError, match="speaker"):
        _call(on, speaker=None)


def test_extend_speakers_keeps_old_rows_and_adds_their_mean():
    model = _multi()
    old = model.speaker_embedding.weight.detach().clone()
    checkpoint = {k: v.clone() for k, v in model.state_dict().items()}
    first = model.extend_speakers(3)
    assert model.speaker_embedding.weight.requires_grad
    table = model.speaker_embedding.weight.detach()
    assert first == 4 and tuple(table.shape) == (7, 384)
    assert torch.equal(table[:4], old)
    mean = old.double().mean(dim=0)
    assert all(torch.equal(table[i], table[4]) for i in (5, 6))
    assert float((table[4].double() - mean).abs().max()) <= 2.0 ** -24 * float(mean.abs().max())
    assert list(model.state_dict()) == list(checkpoint) and tuple(model.state_dict()["speaker_embedding.weight"].shape) == (7, 384)
    assert model.extend_speakers(1) == 7
    # a checkpoint of the smaller table: load_state_dict refuses the shape, load(ignore_mismatched_keys=True) keeps the grown table
    with pytest.raises(RuntimeError, match="size mismatch"):
        model.load_state_dict(checkpoint)
    grown = model.speaker_embedding.weight.detach().clone()
    model.load(checkpoint, ignore_mismatched_keys=True)
    assert torch.equal(model.speaker_embedding.weight, grown)
    model.freeze(["speaker_embedding"])
    assert [n for n, p in model.named_parameters() if p.requires_grad] == ["speaker_embedding.weight"]
    with pytest.raises(ValueError):
        AcousticModel.init(AcousticDims().model_config()).extend_speakers(1)
    with pytest.raises(ValueError):
        model.extend_speakers(0)


def test_batch_ingest_passes_speaker_through_only_when_present():
    ing = ingest.BatchIngest("cpu", max_batch=8, max_text=40, max_mel=96, slots=2)
    batches = []
    for k, (b, l, m) in enumerate([(8, 40, 96), (3, 17, 50), (5, 40, 33)]):
        inp = synth.make_inputs(b, l, m, variable=True, seed=k)
        batches.append({"text_vector": inp["text"], "text_vector_len": inp["text_len"], "mel": inp["mel"],
                        "mel_len": inp["mel_len"], "pitch": inp["pitch"], "energy": inp["energy"]})
    batches[0]["speaker"] = torch.arange(8).view(8, 1) * 100
    batches[2]["speaker"] = torch.tensor([[4], [0], [1306], [2], [2]])
    plain = {"text", "text_len", "mel", "mel_len", "pitch", "energy"}
    for k in range(3):                    # slot 0 holds a batch with ids, then one without (batch 1 goes to slot 1), then with again
        ing.submit(batches[k])
        got = ing.get()
        assert set(got) == set(batches[k])
        for name, t in batches[k].items():
            assert got[name].shape == t.shape and got[name].dtype == t.dtype and torch.equal(got[name], t), name
        kw = ingest.model_inputs(got)
        assert set(kw) == (plain | {"speaker"} if "speaker" in batches[k] else plain)
        if "speaker" in kw:
            assert kw["speaker"] is got["speaker"]
        ing.done()
    ing.submit(dict(batches[1], speaker=None))                                   # the collator's field of single-speaker data
    assert "speaker" not in ing.get()
    ing.done()
    with pytest.raises(AssertionError):
        ing.submit(dict(batches[1], speaker=torch.zeros(3, 1, dtype=torch.int32)))


def test_the_fixture_matches_its_inputs_and_its_exact_zeros():
    g = golden("speaker_train.npz")
    inp = hdr.fixture_inputs()
    assert [crc(inp[k]) for k in ("text", "mel", "pitch", "energy")] == [int(v) for v in g["inputs_crc"]]
    assert g["speaker"].tolist() == [[3], [1]] and g["absent"].tolist() == [0, 2]
    names = [str(n) for n in g["names"]]
    model = _multi()
    assert names == [n for n, _ in model.named_parameters()] and len(names) == 207
    for tag in ("soft", "hard"):
        table = g[f"{tag}_table_grad"]
        assert table.shape == (4, 384) and table.dtype == np.float32
        assert not table[[0, 2]].any() and table[1].any() and table[3].any()
        i = names.index("speaker_embedding.weight")
        assert abs(float(np.linalg.norm(table.astype(np.float64))) - float(g[f"{tag}_grad_norm"][i])) <= 1e-12
        assert g[f"{tag}_grad_norm"].shape == (207,) and float(g[f"{tag}_d_table"]) < 1e-6
    assert g["mel_rows"].shape == (2, 80, 512 // int(g["mel_row_step"])) and g["dec_lengths"].tolist() == [512, 390]
    assert float(g["mel_moved"]) > 0.1
