#!/usr/bin/env python3
"""Time of the noise reducer (ispk_noise_profile_f64 and ispk_noise_reduce_f32, csrc/noise.hip) inside a captured
graph on 64 items of 131,072 samples (speech-like bursts of 0.3 s between pauses of 0.25 s, white noise of 1e-3 everywhere), the
profile and the reduce apart, beside in the same run
  * the vocoder denoiser on the same batch (ispk_denoise_f32: the same tile without the gain rows and the halo transforms);
  * the screen's spectrum pass (parts = 2: every frame transformed once, float64 partials - the profile transforms the noise
    frames only);
  * Segmenter.plan (the hop sums and a per-item pass: what the profile does before its transforms);
  * the reduce without smoothing (smooth_frames = smooth_bins = 0: no halo transforms, one gain row read per bin);
  * the traffic floor of the reduce at 6.3 TB/s (the memory rate the other sections of DESIGN.md use): every sample read and
    written once and 1,024 + 512 smooth_frames more read per tile of 4,096.
Device time from HIP events; `--reps` calls captured into one HIP graph and replayed; median of `--rounds` rounds.  One JSON
line.  Nothing is asserted.

    python tools/time_noise.py [--reps 10] [--rounds 5] [--items 64] [--samples 131072]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, runtime  # noqa: E402
from isp_tts_amd.data import NoiseReducer, Screen, Segmenter  # noqa: E402
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


def recordings(B, S, dev):
    """Bursts of three harmonics (another pitch per item) under a raised-cosine gate, 0.3 s on and 0.25 s off, plus white noise."""
    t = torch.arange(S, dtype=torch.float32, device=dev) / RATE
    period, on = 0.55, 0.3
    phase = torch.remainder(t, period)
    gate = ((phase < on).float() * torch.clamp(torch.minimum(phase, on - phase) / 0.005, 0.0, 1.0))
    x = torch.empty((B, S), dtype=torch.float32, device=dev)
    for b in range(B):
        f0 = 110.0 + 5.0 * b
        tone = sum(a * torch.sin(2.0 * torch.pi * h * f0 * t) for h, a in ((1, 1.0), (2, 0.5), (3, 0.25)))
        x[b] = 0.3 * gate * tone
    return x + 1e-3 * torch.randn((B, S), dtype=torch.float32, device=dev)


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
    nr = NoiseReducer(RATE)
    raw = NoiseReducer(RATE, smooth_frames=0, smooth_bins=0)
    out = nr.empty_outputs(B, dev, samples=S)
    for m in (nr, raw):
        m.device_tables(dev)
    r = nr(x, lens, out=out)
    torch.cuda.synchronize()
    noise_frames = r["noise_frames"].cpu().tolist()
    flags = r["flags"].cpu().tolist()
    pause = ((x - r["audio"]) ** 2).mean().sqrt().item()
    noise = r["noise"].clone()
    y = torch.empty_like(x)
    denoiser = Denoiser(torch.full((513,), 0.02), strength=1.0).to(dev)
    screen = Screen(RATE)
    screen_out = screen.empty_outputs(B, dev, samples=S)
    screen.device_tables(dev)
    seg = Segmenter(RATE, target_s=1.0, max_s=3.0, min_s=0.5, max_segments=16)
    seg_out = seg.empty_outputs(B, 1, None, dev, recording_samples=S)
    profile = graphed(lambda: nr.profile(x, lens, out=out), a.reps, a.rounds)
    reduce = graphed(lambda: nr.apply(x, lens, noise, out=y), a.reps, a.rounds)
    reduce_raw = graphed(lambda: raw.apply(x, lens, noise, out=y), a.reps, a.rounds)
    both = graphed(lambda: nr(x, lens, out=out), a.reps, a.rounds)
    denoise = graphed(lambda: denoiser(x, lens, out=y), a.reps, a.rounds)
    spectrum = graphed(lambda: screen(x, lens, out=screen_out, parts=2), a.reps, a.rounds)
    plan = graphed(lambda: seg.plan(x, lens, out=seg_out), a.reps, a.rounds)
    tiles = -(-S // runtime.NOISE_TILE_SAMPLES)
    moved = 4.0 * B * (2 * S + (1024 + 512 * nr.smooth_frames) * tiles)
    us = lambda ms: round(ms * 1e3, 1)                                          # noqa: E731
    print(json.dumps({"what": f"{B} x {S}", "frames": B * (1 + S // 256), "noise_frames": sum(noise_frames),
                      "flagged": sum(bool(f) for f in flags), "rms_removed": round(pause, 6), "profile_us": us(profile),
                      "reduce_us": us(reduce), "reduce_unsmoothed_us": us(reduce_raw), "profile_and_reduce_us": us(both),
                      "reduce_traffic_floor_us": round(moved / MEMORY_TB_S / 1e6, 1), "denoiser_us": us(denoise),
                      "screen_spectrum_only_us": us(spectrum), "segmenter_plan_us": us(plan), "reps": a.reps, "rounds": a.rounds}),
          flush=True)


if __name__ == "__main__":
    main()
