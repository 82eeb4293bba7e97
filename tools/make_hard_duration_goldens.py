"""Generates tests/golden/hard_duration.npz: the REFERENCE acoustic model with `soft_duration: False` (its constructor default:
rows repeated round(duration) times, pitch / energy targets plain means over each token's frames) on the B = 2 inputs of
forward.npz / train.npz, with every 7th pitch frame zeroed (tests/hard_duration_reference.py `fixture_inputs`):
`forward`, `infer(steps=4)` batched and for one utterance, and the training step of oracle/make_goldens.py `gen_train`.

CPU only, run from the repository root where the reference exists (not on the GPU box):

    python3 tools/make_hard_duration_goldens.py

The reference is imported read-only through `oracle/ref_shims` like oracle/make_goldens.py does.  Three distances are printed
and stored; the tests use the stored values:
  d_avg         the reference's averager (differences of fp32 running sums) against float64 direct means, pitch and energy
  d_mel         the CPU restatement's teacher-forced mel (tests/hard_duration_reference.py) against the reference's
  infer_margin  the smallest distance of a valid token's predicted duration to a rounding boundary in the reference's `infer`;
                asserted >= 1e-3, so that fp32-level differences of the prediction cannot change a rounded duration and no
                token needs excluding from the exact comparison.  Should new weights or inputs break it: pick other inputs.
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
from tts.models.acoustic.model import AcousticModel  # noqa: E402  (reference)

import hard_duration_reference as hdr  # noqa: E402
from isp_tts_amd import synth  # noqa: E402
from isp_tts_amd.config import AcousticDims  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hard_duration.npz")
torch.set_num_threads(8)


def build_reference(sd):
    model = AcousticModel.init(DictConfig(AcousticDims().model_config(soft_duration=False))).eval()
    assert list(model.state_dict().keys()) == list(sd.keys()), "state_dict keys differ from the soft-duration model's"
    model.load_state_dict(sd, strict=True)
    assert model.temporal_adaptor.soft_duration is False
    return model


def maxdiff(a, b) -> float:
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def gen_forward(model, sd, inp, out):
    print("forward (B=2, L=(100,73), M=(512,390))")
    with torch.no_grad(), _Noise(inp["flow_noise"], inp["flow_time"]):
        ref = model(inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], pitch=inp["pitch"], energy=inp["energy"])
    ao, dur = ref.adaptor_output, ref.aligner_output.attn_hard_duration
    tm = torch.arange(100)[None] < inp["text_len"][:, None]
    d_avg = [maxdiff(ao.pitch_target, hdr.hard_average(inp["pitch"], dur) * tm),
             maxdiff(ao.energy_target, hdr.hard_average(inp["energy"], dur) * tm)]
    mine = hdr.acoustic_forward(sd, inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"], inp["energy"],
                                inp["flow_noise"], inp["flow_time"])
    assert torch.equal(mine.aligner.attn_hard_duration.long(), dur.long()), "the restatement's MAS durations differ"
    assert torch.equal(mine.adaptor.dec_lengths, ao.dec_lengths)
    d_mel = maxdiff(ref.mel, mine.mel)
    print(f"  dec_lengths {ao.dec_lengths.tolist()}; d_avg pitch {d_avg[0]:.3e} energy {d_avg[1]:.3e}; d_mel {d_mel:.3e}; "
          f"flow_loss diff {maxdiff(ao.losses['flow_loss'], mine.adaptor.flow_loss):.3e}")
    out.update(text_len=inp["text_len"].numpy(), mel_len=inp["mel_len"].numpy(),
               inputs_crc=np.array([crc(inp[k]) for k in ("text", "mel", "pitch", "energy")], dtype=np.int64),
               duration_target=dur.long().numpy(), dec_lengths=ao.dec_lengths.numpy(), pitch_target=ao.pitch_target.numpy(),
               energy_target=ao.energy_target.numpy(), mel_rows=ref.mel[:, :, ::hdr.MEL_ROW_STEP].numpy(),
               mel_row_step=np.array(hdr.MEL_ROW_STEP), flow_loss=ao.losses["flow_loss"].numpy(),
               log_duration=ao.log_duration.numpy(), d_avg=np.array(d_avg), d_mel=np.array(d_mel))


def gen_infer(model, sd, inp, out):
    print("infer(steps=4)")
    raws = []
    predictor = model.temporal_adaptor.predictor
    ref_infer = predictor.infer

    def recording_infer(*args, **kw):
        pred = ref_infer(*args, **kw)
        raws.append(torch.exp(pred[..., 0]) - 1)                     # what :354 rounds (duration_factor 1)
        return pred
    predictor.infer = recording_infer
    margins = []
    tm = torch.arange(100)[None] < inp["text_len"][:, None]
    for tag, text, text_len, x_t, valid in (("b2", inp["text"], inp["text_len"], inp["flow_noise"], tm),
                                            ("b1", inp["text"][:1], None, inp["flow_noise"][:1], None)):
        with torch.no_grad(), _Noise(x_t):
            mel_ref, ao = model.infer(text, text_lengths=text_len, steps=4)
        mel_mine, ad, _ = hdr.acoustic_infer(sd, text, text_len, None, x_t, 4)
        margins.append(hdr.half_integer_margin(raws[-1], valid))
        same = torch.equal(ao.duration, ad.duration)
        print(f"  {tag}: dec_lengths {ao.dec_lengths.tolist()}, {int((ao.duration == 0).sum())} zero durations, margin "
              f"{margins[-1]:.3e} over {int(valid.sum()) if valid is not None else raws[-1].numel()} tokens; restatement: durations "
              f"equal {same}, mel diff {maxdiff(mel_ref, mel_mine) if same else float('nan'):.3e}")
        out.update({f"{tag}_duration": ao.duration.numpy(), f"{tag}_dec_lengths": ao.dec_lengths.numpy(),
                    f"{tag}_pitch": ao.pitch.numpy(), f"{tag}_energy": ao.energy.numpy(), f"{tag}_mel": mel_ref.numpy()})
    predictor.infer = ref_infer
    margin = min(margins)
    assert margin >= 1e-3, f"a predicted duration lies {margin:.2e} from a rounding boundary: pick other inputs"
    out["infer_margin"] = np.array(margin)


def gen_train(model, inp, out):
    """oracle/make_goldens.py `gen_train` on the hard-duration model: MAS gets a copy of the logits (on CPU the reference hands
    it a view of the autograd tensor's memory and overwrites it; on its training device it copies - see the comment there)."""
    print("training step")
    from tts.models.acoustic.loss import AcousticModelLoss  # noqa: E402  (reference)
    cpu_mas = type(model.aligner).cpu_binarize_attention_parallel
    model.aligner.cpu_binarize_attention_parallel = lambda logits, tl, ml: cpu_mas(logits.clone(), tl, ml)
    criterion = AcousticModelLoss()
    names = [n for n, _ in model.named_parameters()]
    with torch.enable_grad():
        with _Noise(inp["flow_noise"], inp["flow_time"]):
            outputs = model(inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], pitch=inp["pitch"], energy=inp["energy"])
        loss, losses = criterion({k: inp[k] for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy")}, outputs)
        loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    out.update(names=np.array(names), loss_total=loss.detach().numpy(),
               grad_norm=np.array([grads[n].double().norm().item() for n in names]),
               grad_absmax=np.array([grads[n].abs().max().item() for n in names]))
    for k, v in losses.items():
        out["loss_" + k.replace("/", "_")] = v.detach().numpy()
    for i, n in enumerate(names):
        out[f"g{i}"] = _sample(grads[n])
    print(f"  losses: total {loss.item():.6f} " + " ".join(f"{k}={v.item():.6f}" for k, v in losses.items())
          + f"; {len(names)} gradients, all finite")


if __name__ == "__main__":
    sd = synth.make_state_dict(AcousticDims())
    model = build_reference(sd)
    inp = hdr.fixture_inputs()
    out: dict = {}
    gen_forward(model, sd, inp, out)
    gen_infer(model, sd, inp, out)
    gen_train(model, inp, out)
    np.savez_compressed(OUT, **out)
    print(f"{os.path.basename(OUT)} {os.path.getsize(OUT) / 1e6:.2f} MB")
