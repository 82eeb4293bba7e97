#!/usr/bin/env python3
"""Time of the segmenter (ispk_segment_plan / ispk_segment_gather_f32, csrc/segment.hip) inside a captured
graph, plan and gather apart, for
  * 64 recordings of 131,072 samples (bursts of 1.5 s, pauses of 0.5 s; pieces of 1 .. 3 s),
  * 8 recordings of 2^24 samples (12.7 min at 22.05 kHz; bursts of 4 s, pauses of 0.5 s; the default budget of 6 .. 20 s),
  * one recording of an hour (79,380,000 samples, 310,079 frames) without a pause and with 3,600 of them: what the per-item
    workgroup and its serial choice cost on the longest item anyone feeds it,
beside the traffic floors at 6.3 TB/s (the memory rate the other sections of DESIGN.md use): 4 B read per sample for the plan;
read plus write of the gathered samples for the gather (and, apart, the write of the whole padded output, which the zero fill
makes the gather do).  Device time from HIP events; `--reps` calls captured into one HIP graph and replayed; median of `--rounds`
rounds.  One JSON line per case.  Nothing is asserted.

    python tools/time_segmenter.py [--reps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph  # noqa: E402
from isp_tts_amd.data import Segmenter  # noqa: E402

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


def recordings(B, S, burst_s, pause_s, dev):
    """Noise at 0.25 in bursts, 1e-4 in the pauses; item b is shifted by b / B of a period, so the cuts differ per item."""
    period, burst = int((burst_s + pause_s) * RATE), int(burst_s * RATE)
    x = torch.empty((B, S), dtype=torch.float32, device=dev)
    i = torch.arange(S, device=dev)
    for b in range(B):
        loud = ((i + (b * period) // B) % period) < burst if pause_s > 0 else torch.ones_like(i, dtype=torch.bool)
        x[b] = torch.randn(S, device=dev) * torch.where(loud, 0.25, 1e-4)
    return x


def case(what, seg, x, rows, a):
    dev = x.device
    B, S = x.shape
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    out = seg.empty_outputs(B, rows, None, dev, recording_samples=S)
    r = seg(x, lens, out=out)
    torch.cuda.synchronize()
    used, wanted = int(r["rows"][0]), int(r["rows_wanted"][0])
    gathered = int(r["audio_len"].sum())
    plan_ms = graphed(lambda: seg.plan(x, lens, out=out), a.reps, a.rounds)
    both_ms = graphed(lambda: seg(x, lens, out=out), a.reps, a.rounds)
    gather_ms = both_ms - plan_ms
    us = lambda ms: round(ms * 1e3, 1)                                          # noqa: E731
    floor = lambda nbytes: round(nbytes / MEMORY_TB_S / 1e6, 1)                 # noqa: E731
    print(json.dumps({"what": what, "B": B, "S": S, "frames_per_item": -(-S // 256), "segments": int(r["wanted"].sum()),
                      "max_segments": seg.max_segments, "rows": rows, "rows_used": used, "rows_wanted": wanted,
                      "samples_out": out["audio"].shape[1], "plan_us": us(plan_ms), "plan_floor_us": floor(4.0 * B * S),
                      "gather_us": us(gather_ms), "gather_floor_us": floor(8.0 * gathered),
                      "gather_floor_with_zero_fill_us": floor(4.0 * gathered + 4.0 * out["audio"].numel()),
                      "reps": a.reps, "rounds": a.rounds}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    case("64 x 131072", Segmenter(RATE, target_s=1.0, max_s=3.0, min_s=0.5, max_segments=16), recordings(64, 131072, 1.5, 0.5, dev), 256, a)
    case("8 x 2^24", Segmenter(RATE), recordings(8, 1 << 24, 4.0, 0.5, dev), 1280, a)
    hour = 3600 * RATE
    case("1 hour, no pause", Segmenter(RATE, max_segments=4096), recordings(1, hour, 1.0, 0.0, dev), 1, a)
    case("1 hour, 3600 pauses", Segmenter(RATE, target_s=0.5, max_s=20.0, min_s=0.1, max_segments=4096),
         recordings(1, hour, 0.6, 0.4, dev), 1, a)


if __name__ == "__main__":
    main()
