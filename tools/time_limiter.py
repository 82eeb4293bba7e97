#!/usr/bin/env python3
"""Time of the true-peak look-ahead limiter (ispk_limit_f32, csrc/limiter.hip) at 64 items x 131,072 samples
with the conditioner's bounds and gain, at look-aheads of 33 samples (1.5 ms at 22.05 kHz) and 256 (the largest), beside
  * its traffic floor: every sample read once and written once (67 MB) over 6.3 TB/s (the memory rate the other sections of
    DESIGN.md use), and
  * ispk_audio_apply_f32 on the same buffers: the conditioner's pass that the limiter launch replaces.
Three inputs, because the kernel skips the sliding minimum and the smoothing sum in a tile that holds nothing to limit:
  quiet    noise that stays under the ceiling: no tile limited - the envelope pass alone
  sparse   the same with one peak at twice the ceiling somewhere in every 16,384 samples: a quarter of the tiles or a few
           more (a peak within 2 L of a tile's edge limits its neighbour too) - speech-like
  dense    noise whose peaks reach twice the ceiling everywhere: every tile limited - the worst case
and the measure-only launch (`Limiter.true_peak`).  Device time from HIP events; every figure is `--reps` calls captured into
one HIP graph and replayed, which is what the launch costs inside a captured chain; median of `--rounds` rounds.  One JSON line
per look-ahead.

    python tools/time_limiter.py [--reps 20] [--rounds 5]
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
from isp_tts_amd.data import Limiter  # noqa: E402

MEMORY_TB_S = 6.3


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
    g = np.random.default_rng(0)
    B, S = 64, 131072
    c = Limiter(22050).ceiling
    noise = g.standard_normal((B, S)).astype(np.float32)
    quiet = noise * np.float32(0.1 * c)                                    # sample peaks around half the ceiling
    sparse = quiet.copy()
    # (at random places: a fixed period would put every limited tile on the same few XCDs, which take workgroups in turn)
    at = np.arange(0, S, 16384)[None, :] + g.integers(0, 16384, (B, S // 16384))
    np.put_along_axis(sparse, at, np.float32(2.0 * c), axis=1)
    dense = noise * np.float32(2.0 * c / np.abs(noise).max())
    inputs = {k: torch.from_numpy(v).to(dev) for k, v in (("quiet", quiet), ("sparse", sparse), ("dense", dense))}
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    bounds = torch.tensor([0, S], dtype=torch.int64, device=dev).repeat(B, 1).contiguous()
    gain = torch.ones((B,), dtype=torch.float32, device=dev)
    out, out_len = torch.empty((B, S), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int64, device=dev)
    nbytes = 8.0 * B * S
    apply_ms = graphed(lambda: runtime.audio_apply(inputs["sparse"], bounds, gain, out, out_len), a.reps, a.rounds)
    for ms in (1.5, 256 / 22.05):
        lim = Limiter(22050, lookahead_ms=ms)
        o = lim.empty_outputs(B, S, dev)
        lim.device_tables(dev)
        row = {"what": "limit", "B": B, "S": S, "lookahead": lim.lookahead, "mb_moved": round(nbytes / 1e6, 2),
               "traffic_floor_us": round(nbytes / MEMORY_TB_S / 1e6, 2), "audio_apply_graphed_us": us(apply_ms)}
        for name, x in inputs.items():
            t = graphed(lambda: lim(x, lens, gain=gain, bounds=bounds, out=o), a.reps, a.rounds)
            torch.cuda.synchronize()
            row[f"{name}_graphed_us"] = us(t)
            row[f"{name}_tb_per_s"] = round(nbytes / t / 1e9, 2)
            row[f"{name}_items_limited"] = int((o["reduction"] < 1.0).sum())
        measure = lambda: runtime.limit(inputs["sparse"], lens, lim.device_tables(dev), lim.ceiling, lim.lookahead, gain,      # noqa: E731
                                        true_peak=o["true_peak"], measure_only=True)
        row["measure_only_graphed_us"] = us(graphed(measure, a.reps, a.rounds))
        print(json.dumps({**row, "reps": a.reps, "rounds": a.rounds}), flush=True)


if __name__ == "__main__":
    main()
