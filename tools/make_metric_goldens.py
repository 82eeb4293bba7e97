"""Generates tests/golden/metrics.npz: the REFERENCE evaluator's metrics (models/acoustic/evaluator.py) on the cases of
`synth.METRIC_CASES` and on the reference model's own forward outputs for the B = 2 inputs of forward.npz.

CPU only, run from the repository root where the reference exists (not on the GPU box):

    python3 tools/make_metric_goldens.py

The reference is imported read-only through `oracle/ref_shims` like oracle/make_goldens.py does.  Its torchaudio import is a
shim there, so before `MCD` is built the name `create_dct` inside the reference's evaluator module is replaced by this
project's restatement (isp_tts_amd.acoustic.create_dct), checked here against scipy's orthonormal DCT-II.  The fixture holds
the three values per case and CRCs of the inputs only: the tests regenerate the inputs from synth's keyed streams.
"""
from __future__ import annotations

import os
import sys
import types
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(1, "/root/reference")

import scipy.fft  # noqa: E402
from tts.models.acoustic import evaluator as ref_evaluator  # noqa: E402  (reference)

from isp_tts_amd import synth  # noqa: E402
from isp_tts_amd.acoustic import create_dct  # noqa: E402
from isp_tts_amd.config import AcousticDims  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metrics.npz")
KEYS = ("metrics/mcd_13", "metrics/alignment_length", "metrics/alignment_strength")
torch.set_grad_enabled(False)


def crc(t) -> int:
    a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def reference_metrics(evaluator, mel_out, mel_target, mel_len, text_len, attn_soft) -> np.ndarray:
    inputs = types.SimpleNamespace(mel=mel_target, mel_len=mel_len, text_len=text_len)
    outputs = types.SimpleNamespace(mel=mel_out, aligner_output=types.SimpleNamespace(attn_soft=attn_soft))
    m = evaluator(inputs, outputs)
    return np.array([float(m[k]) for k in KEYS], dtype=np.float32)


def forward_case(evaluator):
    """The reference model's forward on forward.npz's inputs (oracle/make_goldens.py:gen_forward)."""
    from oracle.make_goldens import _Noise, build_reference
    model, _ = build_reference(AcousticDims())
    inp = synth.make_inputs(2, 100, 512)
    text_len, mel_len = torch.tensor([100, 73]), torch.tensor([512, 390])
    tm = torch.arange(100)[None] < text_len[:, None]
    mm = torch.arange(512)[None] < mel_len[:, None]
    text, mel = inp["text"] * tm, inp["mel"] * mm[:, None]
    pitch, energy = inp["pitch"] * mm, inp["energy"] * mm
    with _Noise(inp["flow_x0"], inp["flow_t"]):
        ref = model(text, text_len, mel, mel_len, pitch=pitch, energy=energy)
    vals = reference_metrics(evaluator, ref.mel, mel, mel_len, text_len, ref.aligner_output.attn_soft)
    crcs = np.array([crc(text), crc(mel), crc(pitch), crc(energy), crc(mel_len), crc(text_len)], dtype=np.int64)
    return vals, crcs


def main():
    dct = create_dct(13, 80)
    sc = scipy.fft.dct(np.eye(80), norm="ortho")[:, :13]          # row n = the DCT-II of e_n: [n_mels, n_mfcc]
    err = np.abs(dct.double().numpy() - sc).max()
    print(f"create_dct(13, 80, 'ortho') vs scipy.fft.dct: max |diff| = {err:.2e}")
    assert err < 1e-7
    ref_evaluator.create_dct = create_dct                          # the reference module's torchaudio name
    evaluator = ref_evaluator.AcousticModelEvaluator(model=None)
    out = {}
    for case in synth.METRIC_CASES:
        d = synth.make_metric_inputs(case)
        out[f"{case}_values"] = reference_metrics(evaluator, d["mel_out"], d["mel_target"], d["mel_len"], d["text_len"],
                                                  d["attn_soft"])
        out[f"{case}_crc"] = np.array([crc(d[k]) for k in ("mel_out", "mel_target", "attn_soft", "mel_len", "text_len")],
                                      dtype=np.int64)
        print(f"{case:8s} {out[f'{case}_values']}")
    out["forward_values"], out["forward_crc"] = forward_case(evaluator)
    print(f"forward  {out['forward_values']}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
