#!/usr/bin/env python3
"""Time of audio conditioning at B = 64 utterances of 131,072 samples at 22,050 Hz: the three launches of
ispk_audio_measure_f64, the one of ispk_audio_apply_f32 and the one of ispk_pcm16, each beside its HBM traffic floor (the
bytes it has to move at 8.0 TB/s), with data.Resampler (48 kHz -> 22.05 kHz, the same output batch) for scale.  Each step is
captured as a HIP graph after a warm-up; device time from HIP events over `--reps` back-to-back replays, median of `--rounds`
rounds; one JSON line.

    python tools/time_conditioning.py [--batch 64] [--samples 131072] [--rate 22050] [--reps 50] [--rounds 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_conditioning.py          # the five kernels one by one

Traffic counted: measure reads the batch twice (once per pass: cond_chunk_kernel and cond_meter_kernel) and writes and
reads 32 bytes of chunk state per 32 samples; apply reads and writes the batch once; PCM16 reads 4 and writes 2 bytes per
sample."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, synth  # noqa: E402
from isp_tts_amd.data import AudioConditioner, Resampler, to_pcm16  # noqa: E402
from isp_tts_amd import runtime  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(fn, reps, rounds):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_conditioning.py measures on the GPU; there is none here")
    B, S = a.batch, a.samples
    kinds = ("harmonic", "chirp", "noise", "edge_lo")
    base = [synth.make_clip(kinds[i % 4], S, 0.1 + 0.1 * i, seed=i, sample_rate=a.rate) for i in range(8)]
    for i, x in enumerate(base):                                     # leading and trailing silence of differing lengths
        x[:1000 * i] = 0.0
        x[S - 1500 * i:] = 0.0
    audio = torch.stack([base[i % 8] for i in range(B)]).cuda()
    alen = torch.full((B,), S, dtype=torch.int64).cuda()
    cond = AudioConditioner(a.rate)
    out = cond.empty_outputs(B, S, "cuda")
    table = cond.device_tables("cuda")
    pcm = torch.empty((B, S), dtype=torch.int16, device="cuda")

    def measure():
        runtime.audio_measure(audio, alen, table, cond.sample_rate, cond.trim_mode, cond.trim_threshold, cond.pad_frames, 1,
                              cond.target_lufs, cond.peak_limit, out["bounds"], out["loudness"], out["peak"], out["gain"])

    def chain():
        r = cond(audio, alen, out=out)
        return to_pcm16(r["audio"], r["audio_len"], out=pcm)

    steps = {"measure": (measure, 4.0 * 2 * B * S + 2.0 * B * S),
             "apply": (lambda: runtime.audio_apply(audio, out["bounds"], out["gain"], out["audio"], out["audio_len"]), 4.0 * 2 * B * S),
             "pcm16": (lambda: to_pcm16(out["audio"], out["audio_len"], out=pcm), 6.0 * B * S),
             "pcm16_dither": (lambda: to_pcm16(out["audio"], out["audio_len"], dither=True, seed=1, out=pcm), 6.0 * B * S),
             "all_three": (chain, 4.0 * 4 * B * S + 2.0 * B * S + 6.0 * B * S)}
    rs = Resampler(48000, a.rate)
    S_in = S * rs.o // rs.n
    wide = torch.stack([synth.make_clip(kinds[i % 4], S_in, 0.5, seed=i, sample_rate=48000) for i in range(8)] * (B // 8 + 1))[:B].cuda()
    wlen = torch.full((B,), S_in, dtype=torch.int64).cuda()
    rout = rs.empty_outputs(B, S_in, "cuda")
    steps["resample_48000"] = (lambda: rs(wide, wlen, out=rout), 4.0 * (wide.numel() + rout[0].numel()))
    res = {"batch": B, "samples": S, "rate": a.rate, "batch_MB": 4.0 * B * S / 1e6, "device": torch.cuda.get_device_name(0)}
    for name, (fn, nbytes) in steps.items():
        g = graph.GraphedCall(fn, warmup=3)
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        ms = timed(g.replay, a.reps, a.rounds)
        floor_us = nbytes / HBM_BYTES_PER_S * 1e6
        res[name] = {"us": 1e3 * ms, "traffic_MB": nbytes / 1e6, "floor_us": floor_us, "of_floor": floor_us / (1e3 * ms)}
    res["kept_samples_mean"] = float(out["audio_len"].double().mean())
    res["loudness_mean"] = float(out["loudness"].mean())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
