#!/usr/bin/env python3
"""Time of the declipper (ispk_declip_f64, csrc/declip.hip) inside a captured graph on 64 items of 131,072
samples: a voiced-speech-like signal (120 Hz with vibrato, 29 harmonics, a slow envelope, a little noise) at a peak of 0.45, twice as
loud and clamped at the rail of 0.5 in
  * no segment of 512 samples (nothing at the rail: every segment is the copy),
  * about 5 % of the segments, at random places,
  * every segment,
beside
  * the traffic floor at 6.3 TB/s (the memory rate the other sections of DESIGN.md use) of one read plus one write of the batch;
    the peak pass reads the batch once more;
  * the screen's levels and runs alone (parts = 1) on the same batch;
  * ispk_audio_apply_f32, the conditioner's plain gain pass (one read, one write), on the same batch.
Device time from HIP events; `--reps` calls captured into one HIP graph and replayed; median of `--rounds` rounds.  One JSON
line.  Nothing is asserted.

    python tools/time_declip.py [--reps 5] [--rounds 5] [--items 64] [--samples 131072]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, runtime  # noqa: E402
from isp_tts_amd.data import Declipper, Screen  # noqa: E402

MEMORY_TB_S = 6.3
RATE, RAIL, H = 22050, 0.5, 512


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


def voices(B, S, dev):
    """fp32 [B, S] at a peak of 0.45 per item."""
    t = torch.arange(S, dtype=torch.float64, device=dev) / RATE
    x = torch.empty((B, S), dtype=torch.float32, device=dev)
    for b in range(B):
        f0 = (100.0 + 2.0 * b) * (1.0 + 0.02 * torch.sin(2 * math.pi * 5.0 * t + 0.3 * b))
        phase = 2 * math.pi * torch.cumsum(f0, 0) / RATE
        y = sum(torch.cos(h * phase + 0.05 * h * h) / h for h in range(1, 30))
        y = y * (0.6 + 0.4 * torch.sin(2 * math.pi * 1.3 * t + b)) + 0.003 * torch.randn(S, dtype=torch.float64, device=dev)
        x[b] = (0.45 * y / y.abs().max()).float()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--samples", type=int, default=131072)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    B, S = a.items, a.samples
    x = voices(B, S, dev)
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    segs = -(-S // H)
    loud = {"none": torch.zeros((B, segs), dtype=torch.bool, device=dev), "sparse": torch.rand((B, segs), device=dev) < 0.05,
            "every": torch.ones((B, segs), dtype=torch.bool, device=dev)}
    dc = Declipper(rail=RAIL)
    out = dc.empty_outputs(B, dev, samples=S)
    row = {"what": f"{B} x {S}", "segments": B * segs, "order": dc.order, "iterations": dc.iterations,
           "traffic_floor_us": round(8.0 * B * S / MEMORY_TB_S / 1e6, 1), "reps": a.reps, "rounds": a.rounds}
    us = lambda ms: round(ms * 1e3, 1)                                          # noqa: E731
    for name, where in loud.items():
        gain = 1.0 + where.repeat_interleave(H, dim=1)[:, :S].float()
        y = (x * gain).clamp_(-RAIL, RAIL).contiguous()
        r = dc(y, lens, out=out)
        torch.cuda.synchronize()
        row[name] = {"loud_segments": int(where.sum()), "clip_samples": int(r["clip_samples"].sum()), "restored": int(r["restored"].sum()),
                     "windows": int(r["windows"].sum()), "dense": int(r["dense"].sum()),
                     "declip_us": us(graphed(lambda: dc(y, lens, out=out), a.reps, a.rounds))}
        if name == "every":
            screen = Screen(RATE, rail=RAIL)
            s_out = screen.empty_outputs(B, dev, samples=S)
            screen.device_tables(dev)
            row["screen_levels_and_runs_us"] = us(graphed(lambda: screen(y, lens, out=s_out, parts=1), a.reps, a.rounds))
            bounds = torch.tensor([0, S], dtype=torch.int64, device=dev).repeat(B, 1).contiguous()
            unit = torch.ones((B,), dtype=torch.float32, device=dev)
            plain, plain_len = torch.empty((B, S), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int64, device=dev)
            row["audio_apply_us"] = us(graphed(lambda: runtime.audio_apply(y, bounds, unit, plain, plain_len), a.reps, a.rounds))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
