#!/usr/bin/env python3
"""Time of the audio front end: data.Resampler (one ispk_resample_f32 launch) at B = 64 utterances of 131,072 OUTPUT samples
for each `--pairs` rate pair, with the fraction of the HBM byte roofline (input + output bytes at 8.0 TB/s), and the
data.DatasetStats launch pair (ispk_feature_stats_f64) at B = 64 x 512 frames.  Device time from HIP events over `--reps`
back-to-back calls, median of `--rounds` rounds; one JSON line.

    python tools/time_audio_frontend.py [--batch 64] [--samples 131072] [--frames 512] [--reps 50] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_audio_frontend.py          # the kernels alone
    python tools/time_audio_frontend.py --cpu --threads 16                                  # CPU figures for scale, no GPU

`--cpu` times, on the host, an fp32 restatement of what the reference runs: torchaudio's resample as a strided conv1d over
the padded waveform (one utterance at a time, as AudioProvider does) and compute_stats' per-utterance loop (torch.quantile,
the two masks, a numpy mean / variance merge)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import synth  # noqa: E402
from isp_tts_amd.data import DatasetStats, Resampler  # noqa: E402
from isp_tts_amd.data.resample import sinc_hann_taps  # noqa: E402

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


def wall(fn, rounds):
    per = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        per.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(per)


def stats_batch(batch, frames):
    d = synth.make_stats_case("voices")
    idx = [i % 64 for i in range(batch)]
    lens = torch.clamp(d["mel_len"][idx], max=frames)
    p, e = d["pitch"][idx, :frames].contiguous(), d["energy"][idx, :frames].contiguous()
    lens[0] = frames
    return p, e, lens


def cpu_resample(x, k, o, n, width):
    """torchaudio's _apply_sinc_resample_kernel: pad (width, width + o), conv1d with the [n, 1, J] kernel at stride o."""
    length = x.shape[-1]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x[None, None], (width, width + o)), k[:, None], stride=o)
    return y.transpose(1, 2).reshape(-1)[: -(-n * length // o)]


def cpu_stats(p, e, lens):
    state = {}
    for b in range(p.shape[0]):
        for name, row in (("pitch", p[b, :lens[b]]), ("energy", e[b, :lens[b]])):
            p25, p75 = torch.quantile(row, 0.25), torch.quantile(row, 0.75)
            x = row[torch.logical_and(row > p25 - 1.5 * (p75 - p25), row < p75 + 1.5 * (p75 - p25))]
            if name == "pitch":
                x = x[x > 0.]
            if len(x) == 0:
                continue
            x = x.numpy()
            m, v, c = np.mean(x), np.var(x), len(x)
            if name in state:
                m0, v0, c0 = state[name]
                mean = (m0 * c0 + m * c) / (c0 + c)
                v = (c0 * (v0 + m0 ** 2) + c * (v + m ** 2)) / (c0 + c) - mean ** 2
                m, c = mean, c0 + c
            state[name] = (m, v, c)
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=131072, help="output samples per utterance")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--pairs", default="48000:22050,44100:22050")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="the CPU restatements only (no GPU needed)")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    res = {"batch": a.batch, "out_samples": a.samples, "frames": a.frames}
    pairs = [tuple(int(v) for v in p.split(":")) for p in a.pairs.split(",")]
    p, e, lens = stats_batch(a.batch, a.frames)
    if a.cpu:
        torch.set_num_threads(a.threads)
        res["threads"] = a.threads
        for orig, new in pairs:
            k, _, o, n, width = sinc_hann_taps(orig, new)
            k32 = torch.from_numpy(k.astype(np.float32))
            S = a.samples * o // n
            waves = [synth.make_clip("noise", S, 0.5, seed=i, sample_rate=orig) for i in range(4)]
            res[f"cpu_resample_{orig}_{new}_ms_per_batch"] = wall(
                lambda: [cpu_resample(waves[i % 4], k32, o, n, width) for i in range(a.batch)], 3)
        res["cpu_stats_ms_per_batch"] = wall(lambda: cpu_stats(p, e, lens.tolist()), 3)
        print(json.dumps(res))
        return
    for orig, new in pairs:
        rs = Resampler(orig, new)
        S = a.samples * rs.o // rs.n
        kinds = synth.CLIP_KINDS
        base = [synth.make_clip(kinds[i % len(kinds)], S, 0.5, seed=i, sample_rate=orig) for i in range(8)]
        audio = torch.stack([base[i % 8] for i in range(a.batch)]).cuda()
        alen = torch.full((a.batch,), S, dtype=torch.int64).cuda()
        out = rs.empty_outputs(a.batch, S, "cuda")
        rs(audio, alen, out=out)
        torch.cuda.synchronize()
        ms = timed(lambda: rs(audio, alen, out=out), a.reps, a.rounds)
        nbytes = 4.0 * (audio.numel() + out[0].numel())
        res[f"resample_{orig}_{new}"] = {"ms": ms, "in_samples": S, "taps": rs.T, "MB": nbytes / 1e6,
                                         "GB_per_s": nbytes / ms / 1e6, "of_hbm_roofline": nbytes / HBM_BYTES_PER_S / (ms * 1e-3)}
        del audio, out
    stats = DatasetStats("cuda")
    pd, ed, ld = p.cuda(), e.cuda(), lens.cuda()
    stats.update(pd, ed, ld)
    torch.cuda.synchronize()
    res["stats_pair_ms"] = timed(lambda: stats.update(pd, ed, ld), a.reps, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
