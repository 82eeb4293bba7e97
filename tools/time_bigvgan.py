#!/usr/bin/env python3
"""Time of the BigVGAN generator (isp_tts_amd.bigvgan.BigVGan, synthetic weights, base unless --dims) at the bench batch
(B = 64 x T = 512 frames) and at B = 8, in fp32 and bf16 compute.  Device time from HIP events over `--reps` back-to-back
calls after warm-up, median of `--rounds` rounds; ms per batch, audio samples/s and the FLOP / HBM-byte counts from the shapes
(every launch's input rows read once, output rows written once, residual / accumulated rows read once; each anti-aliased
activation is a pass of its own: rows read once, written once, 56 FLOPs and two sinf per element).  One JSON line per
configuration.  `--per-kernel` adds, for the B = 64 batch, one line per kernel label with its launches, time, TFLOP/s and
TB/s (HIP events around every launch, runtime.LaunchProfiler).

    python tools/time_bigvgan.py [--reps 5] [--rounds 5] [--per-kernel] [--dims base|odd|odd2]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_bigvgan.py --reps 2 --rounds 1 --only 64 --dtype bf16
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import runtime, synth  # noqa: E402
from isp_tts_amd.bigvgan import BigVGan  # noqa: E402


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


def counts(cfg, B, T, bf16):
    """Algorithmic FLOPs and HBM bytes of one call."""
    R, C = B * T, cfg["upsample_initial_channel"]
    kp = (7 * cfg["n_mels"] + 7) // 8 * 8
    flops = 2.0 * R * kp * C
    nbytes = R * (cfg["n_mels"] * 4 + kp * (2 if bf16 else 4) * 2 + 4 * C)
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        flops += 2.0 * R * C * (C // 2) * k                     # every input row meets k taps
        nbytes += 4 * R * (C + u * C // 2)
        R, C = R * u, C // 2
        for r, D in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            convs = len(D) * (2 if str(cfg["resblock"]) == "1" else 1)
            flops += convs * (2.0 * R * C * C * r + 56.0 * R * C)
            nbytes += convs * 4 * R * C * 4 + len(D) * 4 * R * C      # in + out per activation and convolution, residual per unit
        nbytes += (len(cfg["resblock_kernel_sizes"]) - 1) * 4 * R * C  # the accumulated sum read back
    flops += (14.0 + 56.0) * R * C
    nbytes += 3 * 4 * R * C + 4 * R
    return flops, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dims", default="base", choices=sorted(synth.BIGVGAN_DIMS))
    ap.add_argument("--only", type=int, default=0, help="only this batch size")
    ap.add_argument("--dtype", default="", choices=["", "f32", "bf16"])
    ap.add_argument("--per-kernel", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    cfg = synth.BIGVGAN_DIMS[a.dims]
    voc = BigVGan.from_state_dict(synth.make_bigvgan_state_dict(cfg), cfg).to(dev).eval()
    dtypes = [d for n, d in (("f32", torch.float32), ("bf16", torch.bfloat16)) if a.dtype in ("", n)]
    for B, T in ((64, 512), (8, 512)):
        if a.only and B != a.only:
            continue
        mel = synth.make_vocoder_mel(B, cfg["n_mels"], T).to(dev)
        for dtype in dtypes:
            voc.set_compute_dtype(dtype)
            out = voc.empty_outputs(B, T, dev)
            ms = timed(lambda: voc(mel, out=out), a.reps, a.rounds)
            fl, nb = counts(cfg, B, T, dtype == torch.bfloat16)
            name = str(dtype).split(".")[-1]
            print(json.dumps({"what": f"bigvgan {a.dims}", "B": B, "T": T, "dtype": name, "ms_per_batch": round(ms, 3),
                              "audio_samples_per_s": round(B * T * voc.hop_length / ms * 1e3), "gflop": round(fl / 1e9, 1),
                              "hbm_gb": round(nb / 1e9, 3), "tflops": round(fl / ms / 1e9, 1),
                              "tb_per_s": round(nb / ms / 1e9, 2)}), flush=True)
            if a.per_kernel and B == 64:
                prof = runtime.LaunchProfiler()
                runtime.set_profiler(prof)
                try:
                    voc(mel, out=out)
                    torch.cuda.synchronize()
                finally:
                    runtime.set_profiler(None)
                for label, d in sorted(prof.summary().items(), key=lambda kv: -kv[1]["total_ms"]):
                    print(json.dumps({"kernel": label, "dtype": name, "launches": d["launches"], "ms": round(d["total_ms"], 3),
                                      "tflops": round(d["flops"] / d["total_ms"] / 1e9, 1),
                                      "tb_per_s": round(d["bytes"] / d["total_ms"] / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
