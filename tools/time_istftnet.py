#!/usr/bin/env python3
"""Time of the iSTFTNet generator (isp_tts_amd.istftnet.IstftNet, synthetic weights, c8c8i) beside the HiFi-GAN generator
(V1) in the SAME run, at the bench batch (B = 64 x T = 512 frames), in fp32 and bf16 compute, each call captured into a HIP
graph.  Device time from HIP events around `--reps` back-to-back replays after warm-up (the capture's own warm-up calls and
one replay); the four configurations are alternated inside every one of `--rounds` rounds, and the median, the fastest and the
slowest round are printed: ms per batch, audio samples/s, and the FLOP / HBM-byte counts from the shapes (tools/time_hifigan's
count, with this output layer's).  One JSON line per configuration.

Then the output layer alone, ispk_istftnet_head_f32 on a [B T 64, 128] stage tensor (eager launches between HIP events), beside
its traffic floor: C floats read per row and hop floats written, over the HBM bandwidth a copy reaches on this chip
(6.29 TB/s for a float4 copy) - the kernel is compute-bound, so its FLOP rate is printed as well.

    python tools/time_istftnet.py [--reps 3] [--rounds 5] [--B 64] [--T 512]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, runtime, synth  # noqa: E402
from isp_tts_amd.hifigan import HifiGan  # noqa: E402
from isp_tts_amd.istftnet import IstftNet  # noqa: E402

COPY_TB_PER_S = 6.29


def counts(cfg, B, T, bf16):
    """Algorithmic FLOPs and HBM bytes of one call (tools/time_hifigan.py's count; the iSTFT head when cfg has one)."""
    R, C = B * T, cfg["upsample_initial_channel"]
    kp = (7 * cfg["n_mels"] + 7) // 8 * 8
    flops = 2.0 * R * kp * C
    nbytes = R * (cfg["n_mels"] * 4 + kp * (2 if bf16 else 4) * 2 + 4 * C)
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        flops += 2.0 * R * C * (C // 2) * k
        nbytes += 4 * R * (C + u * C // 2)
        R, C = R * u, C // 2
        for r, D in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            convs = len(D) * (2 if str(cfg["resblock"]) == "1" else 1)
            flops += convs * 2.0 * R * C * C * r
            nbytes += convs * 4 * R * C * 2 + len(D) * 4 * R * C
        nbytes += (len(cfg["resblock_kernel_sizes"]) - 1) * 4 * R * C
    n_fft = cfg.get("gen_istft_n_fft")
    if n_fft:
        hop = cfg["gen_istft_hop_size"]
        flops += R * (14.0 * C * (n_fft + 2) + 2.0 * n_fft * n_fft)
        nbytes += 4 * R * C + 4 * R * hop
    else:
        flops += 14.0 * R * C
        nbytes += 4 * R * C + 4 * R
    return flops, nbytes


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_istftnet.py measures on the GPU; there is none")
    dev, B, T = "cuda:0", a.B, a.T
    mel = synth.make_vocoder_mel(B, 80, T).to(dev)
    runs = []
    for what, cls, cfg, make in (("istftnet c8c8i", IstftNet, synth.ISTFTNET_DIMS["c8c8i"], synth.make_istftnet_state_dict),
                                 ("hifigan v1", HifiGan, synth.HIFIGAN_DIMS["v1"], synth.make_hifigan_state_dict)):
        for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            voc = cls.from_state_dict(make(cfg), cfg).to(dev).eval().set_compute_dtype(dtype)
            out = voc.empty_outputs(B, T, dev)
            g = graph.GraphedCall(lambda voc=voc, out=out: voc(mel, out=out))
            g.replay()
            torch.cuda.synchronize()
            runs.append((what, name, cfg, voc, g, []))
    for _ in range(a.rounds):                        # alternated: every round times all four
        for *_, g, per in runs:
            per.append(events(g.replay, a.reps))
    for what, name, cfg, voc, g, per in runs:
        ms = statistics.median(per)
        fl, nb = counts(cfg, B, T, name == "bfloat16")
        print(json.dumps({"what": what, "B": B, "T": T, "dtype": name, "graph": True, "ms_per_batch": round(ms, 3),
                          "ms_min": round(min(per), 3), "ms_max": round(max(per), 3), "rounds": a.rounds, "reps": a.reps,
                          "audio_samples_per_s": round(B * T * voc.hop_length / ms * 1e3), "gflop": round(fl / 1e9, 1),
                          "hbm_gb": round(nb / 1e9, 3), "tflops": round(fl / ms / 1e9, 1), "tb_per_s": round(nb / ms / 1e9, 2)}),
              flush=True)
    del runs

    # the output layer alone, on the last stage's shape
    cfg = synth.ISTFTNET_DIMS["c8c8i"]
    C, n_fft, hop = cfg["upsample_initial_channel"] >> 2, cfg["gen_istft_n_fft"], cfg["gen_istft_hop_size"]
    Tl = T * 64
    R = B * Tl
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((R, C), device=dev, generator=gen)
    w = torch.randn((7, n_fft + 2, C), device=dev, generator=gen) * (0.25 / (7 * C) ** 0.5)
    bias = torch.zeros((n_fft + 2,), device=dev)
    table = runtime.istftnet_table(n_fft).to(dev)
    audio = torch.empty((B, hop * Tl), device=dev)
    fn = lambda: runtime.istftnet_head(x, Tl, w, bias, table, n_fft, hop, audio)
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    head_reps = 100 * a.reps                        # a millisecond kernel: a window of a few hundred ms, as the models get
    per = [events(fn, head_reps) for _ in range(a.rounds)]
    ms = statistics.median(per)
    fl, nb = R * (14.0 * C * (n_fft + 2) + 2.0 * n_fft * n_fft), 4.0 * R * (C + hop)
    print(json.dumps({"kernel": f"istftnet_head_kernel<{n_fft}>", "rows": R, "C": C, "ms": round(ms, 3), "ms_min": round(min(per), 3),
                      "ms_max": round(max(per), 3), "rounds": a.rounds, "reps": head_reps, "gflop": round(fl / 1e9, 1),
                      "tflops": round(fl / ms / 1e9, 1), "hbm_gb": round(nb / 1e9, 3), "tb_per_s": round(nb / ms / 1e9, 2),
                      "traffic_floor_ms": round(nb / COPY_TB_PER_S / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
