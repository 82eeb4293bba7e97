#!/usr/bin/env python3
"""Time of the time stretch (ispk_stretch_f32, csrc/stretch.hip) inside a captured graph on 64 items of 131,072
samples (white noise of 0.1: the work does not depend on the signal) at the rates 0.8, 1.0 and 1.25, with a rate per item on the
device, beside in the same run
  * the vocoder denoiser on the same batch (ispk_denoise_f32: the same tile with one forward and one inverse transform per frame
    and no float64);
  * PitchShift(ratio=(5, 4)): the stretch at 0.8 and the resampler;
  * the traffic floor of the stretch at 6.3 TB/s (the memory rate the other sections of DESIGN.md use): every input sample read
    by the chunk pass and by the tiles (the halo apart), every output sample written once, a phasor row per tile written and
    read twice.
Device time from HIP events; `--reps` calls captured into one HIP graph and replayed; median of `--rounds` rounds.  One JSON
line.  Nothing is asserted.

    python tools/time_stretch.py [--reps 10] [--rounds 5] [--items 64] [--samples 131072]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, runtime  # noqa: E402
from isp_tts_amd.data import PitchShift, TimeStretch  # noqa: E402
from isp_tts_amd.denoiser import Denoiser  # noqa: E402

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
    x = 0.1 * torch.randn((B, S), dtype=torch.float32, device=dev)
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    ts = TimeStretch()
    ts.device_tables(dev)
    us = lambda ms: round(ms * 1e3, 1)                                          # noqa: E731
    res = {"what": f"{B} x {S}", "reps": a.reps, "rounds": a.rounds}
    for rate in (0.8, 1.0, 1.25):
        out_samples = TimeStretch.out_samples(S, rate)
        out = ts.empty_outputs(B, dev, samples=out_samples)
        rates = torch.full((B,), rate, dtype=torch.float64, device=dev)
        r = ts(x, lens, rate=rates, out=out)
        torch.cuda.synchronize()
        assert not r["flags"].any().item() and int(r["audio_len"][0]) == round(S / rate)
        t = graphed(lambda: ts(x, lens, rate=rates, out=out), a.reps, a.rounds)
        tiles = -(-out_samples // runtime.STRETCH_TILE_SAMPLES)
        moved = 4.0 * B * (2 * S + out_samples) + 2.0 * 16.0 * B * tiles * runtime.STRETCH_BINS
        res[f"stretch_{rate}_us"] = us(t)
        res[f"stretch_{rate}_output_frames"] = B * (1 + round(S / rate) // 256)
        res[f"stretch_{rate}_traffic_floor_us"] = round(moved / MEMORY_TB_S / 1e6, 1)
    ps = PitchShift(RATE, ratio=(5, 4))
    ps.device_tables(dev)
    ps_out = ps.empty_outputs(B, S, dev)
    res["pitch_shift_5_4_us"] = us(graphed(lambda: ps(x, lens, out=ps_out), a.reps, a.rounds))
    y = torch.empty_like(x)
    denoiser = Denoiser(torch.full((513,), 0.02), strength=1.0).to(dev)
    res["denoiser_us"] = us(graphed(lambda: denoiser(x, lens, out=y), a.reps, a.rounds))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
