#!/usr/bin/env python3
"""Time of the pitch tracker (ispk_pyin_observe_f32, ispk_pyin_decode_f64, csrc/pyin.hip) inside a captured graph
on 64 items of 131,072 samples (512 frames each): seven harmonics of a gliding tone over a noise floor, a second of silence and a
noise burst per item - the work of the observation depends on the number of troughs, so white noise alone would be the worst case
and a clean tone the best; both are timed too.  Observe and decode separately, then the pair, beside in the same run
  * data.AcousticFeatures on the same batch with the default torch-yin pitch (its one launch: the yardstick), and with
    pitch_method="pyin" (that launch without its pitch, then the tracker's two);
  * per frame figures: the decode's time per (item, frame), since one workgroup walks an item's frames in order.
Device time from HIP events; `--reps` calls captured into one HIP graph and replayed; median of `--rounds` x 4 replays.  One JSON
line.  Nothing is asserted.

    python tools/time_pyin.py [--reps 5] [--rounds 5] [--items 64] [--samples 131072]
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
from isp_tts_amd.data import AcousticFeatures, PitchTracker  # noqa: E402

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


def voices(B, S, dev):
    """Gliding seven-harmonic tones (a base per item between 90 and 250 Hz) over a 1e-2 noise floor, a second of silence at the
    start and a quarter second of noise in the middle."""
    g = torch.Generator(device="cpu").manual_seed(0)
    t = torch.arange(S, dtype=torch.float64) / RATE
    base = 90.0 * (250.0 / 90.0) ** torch.rand((B, 1), generator=g, dtype=torch.float64)
    f = base * 2.0 ** (0.3 * torch.sin(2 * math.pi * 1.3 * t)[None] + 0.01 * torch.sin(2 * math.pi * 5.5 * t)[None])
    phase = 2 * math.pi * torch.cumsum(f, dim=1) / RATE
    x = 0.2 * sum(torch.sin(h * phase) / h for h in range(1, 8))
    x[:, :RATE] = 0.0
    x[:, S // 2:S // 2 + RATE // 4] = 0.1 * torch.randn((B, RATE // 4), generator=g, dtype=torch.float64)
    x += 1e-2 * torch.randn((B, S), generator=g, dtype=torch.float64)
    return x.float().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--samples", type=int, default=131072)
    a = ap.parse_args()
    dev = "cuda:0"
    B, S = a.items, a.samples
    M = runtime.feature_frames(S)
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    tracker = PitchTracker(RATE)
    tw, prior, trans = tracker.device_tables(dev)
    us = lambda ms: round(ms * 1e3, 1)                                          # noqa: E731
    res = {"what": f"{B} x {S}", "frames": B * M, "bins": tracker.n_bins, "width": tracker.width, "reps": a.reps, "rounds": a.rounds}
    g = torch.Generator(device="cpu").manual_seed(1)
    t = torch.arange(S, dtype=torch.float64) / RATE
    signals = {"voices": voices(B, S, dev),
               "noise": (0.1 * torch.randn((B, S), generator=g)).to(dev),
               "tone": (0.3 * torch.sin(2 * math.pi * 220.0 * t)).float().expand(B, S).contiguous().to(dev)}
    out = tracker.empty_outputs(B, S, dev)
    for name, x in signals.items():
        observe = lambda: runtime.pyin_observe(x, lens, tw, prior, out["obs"], out["frames"], tracker.min_period,    # noqa: E731
                                               tracker.max_period, float(RATE), tracker.f_min, tracker.bins_per_semitone)
        decode = lambda: runtime.pyin_decode(out["obs"], out["frames"], trans, tracker.width, tracker.f_min,         # noqa: E731
                                             tracker.bins_per_semitone, out={k: v for k, v in out.items() if k != "obs"})
        r = tracker(x, lens, out=out)
        torch.cuda.synchronize()
        res[f"{name}_voiced_share"] = round(float(r["voiced"].float().mean()), 3)
        res[f"{name}_observe_us"] = us(graphed(observe, a.reps, a.rounds))
        t_dec = graphed(decode, a.reps, a.rounds)
        res[f"{name}_decode_us"] = us(t_dec)
        res[f"{name}_decode_us_per_frame_of_an_item"] = round(t_dec * 1e3 / M, 2)
        res[f"{name}_tracker_us"] = us(graphed(lambda: tracker(x, lens, out=out), a.reps, a.rounds))
    x = signals["voices"]
    for method in ("torch-yin", "pyin"):
        feats = AcousticFeatures(sample_rate=RATE, pitch_method=method, pitch_f_max=880.0 if method == "pyin" else 800)
        feats.device_tables(dev)
        f_out = feats.empty_outputs(B, S, dev)
        feats(x, lens, out=f_out)
        torch.cuda.synchronize()
        res[f"features_{method}_us"] = us(graphed(lambda: feats(x, lens, out=f_out), a.reps, a.rounds))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
