#!/usr/bin/env python3
"""Time of the screen (ispk_screen_f64, csrc/screen.hip) inside a captured graph on 64 items of 131,072 samples
(noise at 0.25 with a clipped stretch, a dropout and a 16 kHz-style empty top band in turn), beside
  * the traffic floor of the audio reads it makes at 6.3 TB/s (the memory rate the other sections of DESIGN.md use): the tile
    pass reads every sample once and 768 more per tile of 4,096, the rail pass every sample once;
  * Segmenter.plan on the same batch (one read of the audio, float64 hop sums, a per-item pass);
  * the screen with the spectrum only (parts = 2: what band_db costs) and with the levels and runs only (parts = 1).
Device time from HIP events; `--reps` calls captured into one HIP graph and replayed; median of `--rounds` rounds.  One JSON
line.  Nothing is asserted.

    python tools/time_screen.py [--reps 10] [--rounds 5] [--items 64] [--samples 131072]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, runtime  # noqa: E402
from isp_tts_amd.data import Screen, Segmenter  # noqa: E402

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


def recordings(B, S, dev):
    x = 0.25 * torch.randn((B, S), dtype=torch.float32, device=dev)
    for b in range(B):
        if b % 4 == 1:
            x[b].clamp_(-0.5, 0.5)                                              # clipped
        elif b % 4 == 2:
            x[b, S // 3:S // 3 + 400] = 0.0                                     # a dropout
        elif b % 4 == 3:
            X = torch.fft.rfft(x[b])
            X[int(len(X) * 8000 / (RATE / 2)):] = 0                             # nothing above 8 kHz
            x[b] = torch.fft.irfft(X, S)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--samples", type=int, default=131072)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    B, S = a.items, a.samples
    x = recordings(B, S, dev)
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    screen = Screen(RATE, min_bandwidth_hz=9000.0)
    out = screen.empty_outputs(B, dev, samples=S)
    screen.device_tables(dev)
    r = screen(x, lens, out=out)
    torch.cuda.synchronize()
    flags = r["flags"].cpu().tolist()
    counts = {name: sum(bool(f & bit) for f in flags) for name, bit in runtime.SCREEN_FLAGS.items()}
    seg = Segmenter(RATE, target_s=1.0, max_s=3.0, min_s=0.5, max_segments=16)
    seg_out = seg.empty_outputs(B, 1, None, dev, recording_samples=S)
    whole = graphed(lambda: screen(x, lens, out=out), a.reps, a.rounds)
    spectrum = graphed(lambda: screen(x, lens, out=out, parts=2), a.reps, a.rounds)
    levels = graphed(lambda: screen(x, lens, out=out, parts=1), a.reps, a.rounds)
    plan = graphed(lambda: seg.plan(x, lens, out=seg_out), a.reps, a.rounds)
    tiles = -(-S // runtime.SCREEN_TILE_SAMPLES)
    read_bytes = 4.0 * B * (2 * S + 768 * tiles)
    us = lambda ms: round(ms * 1e3, 1)                                          # noqa: E731
    print(json.dumps({"what": f"{B} x {S}", "frames": B * ((S - 1024) // 256 + 1), "flagged": counts, "screen_us": us(whole),
                      "audio_read_floor_us": round(read_bytes / MEMORY_TB_S / 1e6, 1), "spectrum_only_us": us(spectrum),
                      "levels_and_runs_only_us": us(levels), "segmenter_plan_us": us(plan), "reps": a.reps, "rounds": a.rounds}), flush=True)


if __name__ == "__main__":
    main()
