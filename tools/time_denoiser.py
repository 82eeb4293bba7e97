#!/usr/bin/env python3
"""Time of the vocoder denoiser (isp_tts_amd.denoiser.Denoiser, one launch of ispk_denoise_f32) at the conditioner's batch
(B = 64 x S = 131,072 samples) and at B = 8, on a 220 Hz sine plus noise with the spectrum's per-bin median as
the bias (about half the bins clamped).  Device time from HIP events over `--reps` back-to-back calls after warm-up, median of
`--rounds` rounds; microseconds per batch, samples/s, the 8 B / sample traffic (read once, write once) as TB/s, and the FLOP
count of the 19 / 16 x two 512-point transforms per hop.  One JSON line per configuration.

    python tools/time_denoiser.py [--reps 20] [--rounds 5] [--only 64] [--ragged]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_denoiser.py --reps 2 --rounds 1 --only 64
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd.denoiser import Denoiser, frame0_magnitude  # noqa: E402


def timed(fn, reps, rounds):
    for _ in range(2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", type=int, default=0, help="only this batch size")
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--ragged", action="store_true", help="lengths spread over [S / 2, S] instead of all S")
    a = ap.parse_args()
    dev, S = "cuda:0", a.samples
    g = np.random.default_rng(0)
    base = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(S) / 22050.0) + 0.1 * g.standard_normal(S)).astype(np.float32)
    frames = np.stack([frame0_magnitude(base[o:o + 2048]) for o in range(0, S - 2048, 4096)])
    den = Denoiser(torch.from_numpy(np.median(frames, axis=0).astype(np.float32)), strength=1.0).to(dev)
    for B in (64, 8):
        if a.only and B != a.only:
            continue
        audio = torch.from_numpy(np.stack([np.roll(base, 37 * b) for b in range(B)])).to(dev)
        lens = torch.full((B,), S, dtype=torch.int64)
        if a.ragged:
            lens = torch.from_numpy(g.integers(S // 2, S + 1, B))
        lens, out = lens.to(dev), torch.empty_like(audio)
        ms = timed(lambda: den(audio, lens, out=out), a.reps, a.rounds)
        n = int(lens.sum())
        flops = n / 256.0 * (19.0 / 16.0) * (2 * 5.0 * 512 * 9 + 40.0 * 513)
        print(json.dumps({"what": "denoiser", "B": B, "S": S, "ragged": bool(a.ragged), "us_per_batch": round(ms * 1e3, 1),
                          "samples_per_s": round(n / ms * 1e3), "hbm_gb": round(8.0 * B * S / 1e9, 4),
                          "tb_per_s": round(8.0 * B * S / ms / 1e9, 2), "gflop": round(flops / 1e9, 2),
                          "tflops": round(flops / ms / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
