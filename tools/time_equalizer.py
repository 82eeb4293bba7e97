#!/usr/bin/env python3
"""Time of the equalizer (ispk_equalize_f32, csrc/equalizer.hip) at 64 items x 131,072 samples with cascades
of N = 1, 4 and 8 sections, beside
  * its traffic floor: every sample read once and written once (8 bytes a sample), the second read that the state launch makes,
    and the state traffic - 2 N doubles written per segment and the w earlier ones read by segment w - over 6.3 TB/s (the
    memory rate the other sections of DESIGN.md use), and
  * ispk_audio_apply_f32 on the same buffers: the plainest pass over a batch that the audio chain has (12.1 us in DESIGN.md 4.27).
Device time from HIP events; every figure is `--reps` calls captured into one HIP graph and replayed, which is what the call
costs inside a captured chain; median of `--rounds` rounds.  One JSON line per N.

    python tools/time_equalizer.py [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, runtime  # noqa: E402
from isp_tts_amd.data import Equalizer, highpass, highshelf, lowpass, lowshelf, notch, peaking  # noqa: E402

MEMORY_TB_S = 6.3
RATE = 22050


def graphed(fn, reps, rounds):
    """Per-call device time in ms of `reps` calls captured into one graph."""
    def many():
        for _ in range(reps):
            fn()
    g = graph.GraphedCall(many)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds * 4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / reps)
    return statistics.median(per)


def us(ms):
    return round(ms * 1e3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    B, S = 64, 131072
    x = torch.from_numpy((0.25 * np.random.default_rng(0).standard_normal((B, S)) + 0.5).astype(np.float32)).to(dev)
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    bounds = torch.tensor([0, S], dtype=torch.int64, device=dev).repeat(B, 1).contiguous()
    gain = torch.ones((B,), dtype=torch.float32, device=dev)
    out, out_len = torch.empty((B, S), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int64, device=dev)
    apply_ms = graphed(lambda: runtime.audio_apply(x, bounds, gain, out, out_len), a.reps, a.rounds)
    bands = [highpass(80.0), peaking(3000.0, 3.0), highshelf(8000.0, -2.0), lowshelf(200.0, 2.0), notch(50.0, 8.0),
             peaking(1000.0, -4.0, 2.0), peaking(5000.0, 2.0), lowpass(10000.0)]
    W = -(-S // runtime.EQ_SEGMENT_SAMPLES)
    for n in (1, 4, 8):
        eq = Equalizer(RATE, bands[:n])
        o = eq.empty_outputs(B, S, dev)
        eq.device_tables(dev)
        state_bytes = 8.0 * 2 * n * B * ((W - 1) + W * (W - 1) / 2)
        nbytes = 8.0 * B * S + 4.0 * B * (S - runtime.EQ_SEGMENT_SAMPLES) + state_bytes
        t = graphed(lambda: eq(x, lens, out=o), a.reps, a.rounds)
        print(json.dumps({"what": "equalize", "B": B, "S": S, "sections": n, "mb_moved": round(nbytes / 1e6, 2),
                          "state_mb": round(state_bytes / 1e6, 3), "traffic_floor_us": round(nbytes / MEMORY_TB_S / 1e6, 2),
                          "floor_8_bytes_a_sample_us": round(8.0 * B * S / MEMORY_TB_S / 1e6, 2),
                          "audio_apply_graphed_us": us(apply_ms), "graphed_us": us(t),
                          "tb_per_s": round(nbytes / t / 1e9, 2), "fp64_fma_per_sample": 12 * n,
                          "fp64_tflops": round(2.0 * 12 * n * B * S / t / 1e9, 2), "reps": a.reps, "rounds": a.rounds}), flush=True)


if __name__ == "__main__":
    main()
