#!/usr/bin/env python3
"""Time of the Vocos vocoder (isp_tts_amd.vocoder.Vocoder, synthetic official-shape weights: 80 mels, dim 512, inter 1536,
8 layers) at the bench batch (B = 64 x T = 512 frames) and at B = 8: a mel of that shape in fp32 and bf16 compute, and
AcousticModel.infer (bf16, 4 Euler steps, 100 tokens -> max_dec_len T) followed by the bf16 vocoder.  Device time from HIP
events over `--reps` back-to-back calls after warm-up, median of `--rounds` rounds; ms per batch, audio samples/s, and the
FLOP / HBM-byte counts from the shapes.  One JSON line per configuration.

    python tools/time_vocoder.py [--reps 20] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_vocoder.py --reps 5 --rounds 1 --no-chain   # kernel stats
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import synth  # noqa: E402
from isp_tts_amd.vocoder import Vocoder  # noqa: E402


def timed(fn, reps, rounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / reps)
    return statistics.median(per)


def counts(B, T, n_mels, dim, inter, layers, bf16):
    """Algorithmic FLOPs and HBM bytes of one call (unfused: every intermediate written once and read once)."""
    R = B * T
    e = 2 if bf16 else 4
    kp = (7 * n_mels + 7) // 8 * 8
    flops = 2.0 * R * (kp * dim + layers * (2 * dim * inter + 7 * dim) + dim * 1032)
    flops += R * 1.25 * (5.0 * 512 * 9 + 20.0 * 513)                             # ISTFT head (FFTs, prologue), recomputed halo
    nbytes = R * (n_mels * 4 + kp * e + 8 * dim + 8 * dim)                       # mel, unfold rows, embedding out + LN
    nbytes += layers * R * (4 * dim + 2 * e * dim + 2 * e * inter + 8 * dim)     # dwconv in, y w+r, hidden w+r, residual r+w
    nbytes += R * (4 * dim + e * dim * 2 + 4 * 1032 * 2) + R * 256 * 4          # final LN, head rows w+r, audio
    return flops, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-chain", action="store_true", help="skip AcousticModel.infer + vocoder")
    a = ap.parse_args()
    dev = "cuda:0"
    dims = synth.VOCODER_DIMS["official"]
    voc = Vocoder.from_state_dict(synth.make_vocoder_state_dict(dims)).to(dev).eval()
    model = None
    for B, T in ((64, 512), (8, 512)):
        mel = synth.make_vocoder_mel(B, dims[0], T).to(dev)
        for dtype in (torch.float32, torch.bfloat16):
            voc.set_compute_dtype(dtype)
            out = voc.empty_outputs(B, T, dev)
            ms = timed(lambda: voc(mel, out=out), a.reps, a.rounds)
            fl, nb = counts(B, T, *dims, dtype == torch.bfloat16)
            print(json.dumps({"what": "vocoder", "B": B, "T": T, "dtype": str(dtype).split(".")[-1], "ms_per_batch": round(ms, 4),
                              "audio_samples_per_s": round(B * T * 256 / ms * 1e3), "gflop": round(fl / 1e9, 1),
                              "hbm_gb": round(nb / 1e9, 3), "tflops": round(fl / ms / 1e9, 1),
                              "tb_per_s": round(nb / ms / 1e9, 2)}), flush=True)
        if a.no_chain:
            continue
        if model is None:
            from isp_tts_amd.acoustic import AcousticModel
            from isp_tts_amd.config import AcousticDims
            model = AcousticModel.init(AcousticDims().model_config()).eval()
            model.load_state_dict(synth.make_state_dict(), strict=True)
            model = model.to(dev).requires_grad_(False).set_compute_dtype(torch.bfloat16)
        voc.set_compute_dtype(torch.bfloat16)
        inp = synth.make_inputs(B, 100, T, variable=False, seed=3)
        text, tl, x0 = inp["text"].to(dev), inp["text_len"].to(dev), inp["flow_x0"].to(dev)
        out = voc.empty_outputs(B, T, dev)

        def chain():
            mel_out, ao = model.infer(text, text_lengths=tl, steps=4, flow_noise=x0, max_dec_len=T)
            return voc(mel_out, ao.dec_lengths if B > 1 else None, out=out)

        ms_chain = timed(chain, a.reps, a.rounds)
        ms_infer = timed(lambda: model.infer(text, text_lengths=tl, steps=4, flow_noise=x0, max_dec_len=T), a.reps, a.rounds)
        print(json.dumps({"what": "infer+vocoder", "B": B, "T": T, "dtype": "bfloat16", "ms_per_batch": round(ms_chain, 4),
                          "infer_alone_ms": round(ms_infer, 4), "audio_samples_per_s": round(B * T * 256 / ms_chain * 1e3)}),
              flush=True)


if __name__ == "__main__":
    main()
