"""Generates tests/golden/speaker_train.npz: the REFERENCE acoustic model with a 4-entry speaker table run through `forward` and
one training step, which it cannot do as written - its `forward` reads `self.speaker_encoder` (model.py:145-146), an attribute
no AcousticModel has.  The tool makes that name an alias of `speaker_embedding` on the instance (`object.__setattr__`: no module
is registered, `state_dict()` is unchanged - asserted), which is what the line means, and what `speaker_in_forward` builds here.

Inputs: the B = 2 batch of tests/hard_duration_reference.py `fixture_inputs` (text_len 100 / 73), speaker ids [[3], [1]], the
synthetic weights plus `synth.make_speaker_table(4)`.  Stored, recorded results only:
  soft durations (the recipes' mode): the teacher-forced `forward` (every second mel frame, log_duration, flow_loss,
      dec_lengths) and the training step as oracle/make_goldens.py `gen_train` stores it (four losses, the total, per tensor
      a norm, the largest entry and a strided sample: 207 tensors), the table's gradient whole (4 x 384);
  hard durations: the losses, the per-tensor norms and largest entries, the table's gradient whole.

CPU only, run from the repository root where the reference exists (not on the GPU box):

    python3 tools/make_speaker_train_goldens.py

Asserted: rows 0 and 2 of the table's gradient (speakers absent from the batch) are exactly zero, and so is the gradient that
arrives at `enc_out + speaker` on every padded row (l >= text_len[b]) - the reason the table-gradient kernel may leave those rows
out.  Printed and stored: the distance between the table's gradient and the float64 sum of that arriving gradient over each
speaker's rows, and how far ids [[3], [3]] move the teacher-forced mel (the ids are read).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.make_goldens import _Noise, _sample, crc  # noqa: E402  (also puts the reference and its shims on sys.path)
from omegaconf import DictConfig  # noqa: E402  (shim)
from tts.models.acoustic.loss import AcousticModelLoss  # noqa: E402  (reference)
from tts.models.acoustic.model import AcousticModel  # noqa: E402  (reference)

import hard_duration_reference as hdr  # noqa: E402
from isp_tts_amd import synth  # noqa: E402
from isp_tts_amd.config import AcousticDims  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "speaker_train.npz")
SPEAKERS = 4
SPEAKER = torch.tensor([[3], [1]])
OTHER = torch.tensor([[3], [3]])
ABSENT = (0, 2)
torch.set_num_threads(8)


def build_reference(sd, soft: bool):
    model = AcousticModel.init(DictConfig(dict(AcousticDims().model_config(soft_duration=soft), num_speakers=SPEAKERS))).eval()
    keys = list(model.state_dict().keys())
    assert set(keys) == set(sd.keys()), "state_dict keys differ"
    object.__setattr__(model, "speaker_encoder", model.speaker_embedding)       # model.py:146 reads this name
    assert list(model.state_dict().keys()) == keys, "the alias changed the state_dict"
    model.load_state_dict(sd, strict=True)
    assert model.temporal_adaptor.soft_duration is soft
    # MAS gets a copy of the logits, as on the reference's training device (see oracle/make_goldens.py `gen_train`)
    cpu_mas = type(model.aligner).cpu_binarize_attention_parallel
    model.aligner.cpu_binarize_attention_parallel = lambda logits, tl, ml: cpu_mas(logits.clone(), tl, ml)
    return model


def run_forward(model, inp, speaker):
    with torch.no_grad(), _Noise(inp["flow_noise"], inp["flow_time"]):
        return model(inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], pitch=inp["pitch"], energy=inp["energy"],
                     speaker=speaker)


def gen_forward(model, inp, out):
    ref, other = run_forward(model, inp, SPEAKER), run_forward(model, inp, OTHER)
    ao = ref.adaptor_output
    moved = float((ref.mel[1] - other.mel[1]).abs().max())
    assert torch.equal(ref.mel[0], other.mel[0]) and moved > 0.1
    print(f"  forward: dec_lengths {ao.dec_lengths.tolist()}, flow_loss {float(ao.losses['flow_loss']):.6f}; ids [[3],[3]] move "
          f"the mel of item 1 by {moved:.3f}")
    out.update(mel_rows=ref.mel[:, :, ::hdr.MEL_ROW_STEP].numpy(), mel_row_step=np.array(hdr.MEL_ROW_STEP),
               log_duration=ao.log_duration.numpy(), flow_loss=ao.losses["flow_loss"].numpy(), dec_lengths=ao.dec_lengths.numpy(),
               mel_moved=np.array(moved))


def gen_train(model, inp, out, tag: str, samples: bool):
    criterion = AcousticModelLoss()
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == 207 and "speaker_embedding.weight" in names
    seen = {}

    def keep(_module, _args, kwargs):           # the tensor `enc_out + speaker` as the adaptor receives it
        seen["x"] = kwargs["enc_out"]
        kwargs["enc_out"].retain_grad()
    handle = model.temporal_adaptor.register_forward_pre_hook(keep, with_kwargs=True)
    model.zero_grad(set_to_none=True)
    with torch.enable_grad():
        with _Noise(inp["flow_noise"], inp["flow_time"]):
            outputs = model(inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], pitch=inp["pitch"], energy=inp["energy"],
                            speaker=SPEAKER)
        loss, losses = criterion({k: inp[k] for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy")}, outputs)
        loss.backward()
    handle.remove()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    table, d_x = grads["speaker_embedding.weight"], seen["x"].grad
    pad = torch.arange(d_x.shape[1])[None] >= inp["text_len"][:, None]
    assert not d_x[pad].any(), "the gradient arriving at enc_out + speaker is not zero on padded rows"
    assert all(not table[s].any() for s in ABSENT), "a speaker absent from the batch has a gradient"
    want = torch.zeros(SPEAKERS, d_x.shape[2], dtype=torch.float64).index_add_(0, SPEAKER.view(-1), d_x.double().sum(dim=1))
    d_table = float((table.double() - want).abs().max())
    print(f"  {tag} step: total {loss.item():.6f} " + " ".join(f"{k}={v.item():.6f}" for k, v in losses.items())
          + f"; {len(names)} gradients, all finite; padded rows and table rows {ABSENT} exactly zero; table gradient vs float64 row "
          f"sums {d_table:.3e} (largest entry {float(table.abs().max()):.3e})")
    out.update({f"{tag}_loss_total": loss.detach().numpy(), f"{tag}_table_grad": table.numpy(), f"{tag}_d_table": np.array(d_table),
                f"{tag}_grad_norm": np.array([grads[n].double().norm().item() for n in names]),
                f"{tag}_grad_absmax": np.array([grads[n].abs().max().item() for n in names])})
    for k, v in losses.items():
        out[f"{tag}_loss_" + k.replace("/", "_")] = v.detach().numpy()
    if samples:
        for i, n in enumerate(names):
            out[f"{tag}_g{i}"] = _sample(grads[n])
    return names


if __name__ == "__main__":
    sd = synth.make_state_dict(AcousticDims())
    sd["speaker_embedding.weight"] = synth.make_speaker_table(SPEAKERS)
    inp = hdr.fixture_inputs()
    out: dict = {"inputs_crc": np.array([crc(inp[k]) for k in ("text", "mel", "pitch", "energy")], dtype=np.int64),
                 "speaker": SPEAKER.numpy(), "absent": np.array(ABSENT)}
    print("soft durations")
    soft = build_reference(sd, True)
    gen_forward(soft, inp, out)
    out["names"] = np.array(gen_train(soft, inp, out, "soft", samples=True))
    print("hard durations")
    gen_train(build_reference(sd, False), inp, out, "hard", samples=False)
    np.savez_compressed(OUT, **out)
    print(f"{os.path.basename(OUT)} {os.path.getsize(OUT) / 1e6:.2f} MB")
