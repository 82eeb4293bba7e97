#!/usr/bin/env python3
"""Time of the Griffin-Lim mel inversion (isp_tts_amd.griffinlim.GriffinLim) at the conditioner's batch (B = 64 x S = 131,072
samples = 512 frames) and at B = 8, on the magnitude of a 220 Hz sine plus noise: one launch of
ispk_griffinlim_step_f32 in mode step, one in mode init, the mel -> magnitude product, and a whole 32-iteration call from mel.
With --momentum M also the fast iteration (FastGriffinLim): one launch of ispk_griffinlim_fast_step_f32 (12 B / sample of audio)
with its time over the plain step's of the same run, the two launches of ispk_griffinlim_error_f32, and a whole fast call.
Device time from HIP events over `--reps` back-to-back calls after warm-up, median of `--rounds` rounds; microseconds per
batch, and for the step the 8 B / sample of audio plus the magnitude read (513 / 256 x 4 B / sample) as TB/s and the FLOP count
of the 20 / 16 x two 512-point transforms per hop.  One JSON line per configuration.

    python tools/time_griffinlim.py [--reps 20] [--rounds 5] [--only 64] [--ragged] [--momentum 0.99]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_griffinlim.py --reps 2 --rounds 1 --only 64
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import runtime  # noqa: E402
from isp_tts_amd.data import AcousticFeatures  # noqa: E402
from isp_tts_amd.griffinlim import FastGriffinLim, GriffinLim  # noqa: E402


def timed(fn, reps, rounds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", type=int, default=0, help="only this batch size")
    ap.add_argument("--samples", type=int, default=131072)
    ap.add_argument("--n-iter", type=int, default=32)
    ap.add_argument("--ragged", action="store_true", help="lengths spread over [T / 2, T] instead of all T")
    ap.add_argument("--momentum", type=float, default=None, help="also time the fast iteration at this momentum")
    a = ap.parse_args()
    dev, S = "cuda:0", a.samples // 256 * 256
    T = S // 256
    g = np.random.default_rng(0)
    base = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(S) / 22050.0) + 0.1 * g.standard_normal(S)).astype(np.float32)
    feats = AcousticFeatures(pitch=False, energy=False)
    gl = GriffinLim.from_features(feats, n_iter=a.n_iter).to(dev)
    for B in (64, 8):
        if a.only and B != a.only:
            continue
        audio = torch.from_numpy(np.stack([np.roll(base, 37 * b) for b in range(B)])).to(dev)
        lens = torch.full((B,), T, dtype=torch.int64)
        if a.ragged:
            lens = torch.from_numpy(g.integers(T // 2, T + 1, B))
        lens = lens.to(dev)
        mel = feats(audio, lens * 256)["mel"]
        mag = gl.magnitude(mel, lens)
        out, other = gl.empty_outputs(B, T, dev), torch.empty_like(audio)
        n = int(lens.sum()) * 256
        step = lambda: runtime.griffinlim_step(audio, mag, lens, gl.tables, other)                       # noqa: E731
        init = lambda: runtime.griffinlim_step(None, mag, lens, gl.tables, other, mode=runtime.GRIFFINLIM_INIT)   # noqa: E731
        whole = lambda: gl(mel, lens, out=out)                                                            # noqa: E731
        to_mag = lambda: gl.magnitude(mel, lens, out=mag)                                                 # noqa: E731
        rows = [("step", step, a.reps), ("init", init, a.reps), ("mel_to_linear", to_mag, a.reps),
                (f"call_{a.n_iter}_iterations", whole, max(1, a.reps // 10))]
        if a.momentum is not None:
            fast = FastGriffinLim.from_features(feats, n_iter=a.n_iter, momentum=a.momentum).to(dev)
            alpha = a.momentum / (1.0 + a.momentum)
            older, sc, work = torch.roll(audio, 1, 0), torch.empty(B, device=dev), torch.empty((B, T, 2), device=dev)
            fast_step = lambda: runtime.griffinlim_fast_step(audio, older, alpha, mag, lens, gl.tables, other)   # noqa: E731
            error = lambda: runtime.griffinlim_error(audio, mag, lens, gl.tables, out=sc, work=work)             # noqa: E731
            fast_whole = lambda: fast(mel, lens, out=out)                                                         # noqa: E731
            rows += [("fast_step", fast_step, a.reps), ("error", error, a.reps),
                     (f"fast_call_{a.n_iter}_iterations", fast_whole, max(1, a.reps // 10))]
        step_ms = None
        for what, fn, reps in rows:
            ms = timed(fn, reps, a.rounds)
            rec = {"what": f"griffinlim {what}", "B": B, "S": S, "ragged": bool(a.ragged), "us_per_batch": round(ms * 1e3, 1),
                   "samples_per_s": round(n / ms * 1e3)}
            if what in ("step", "fast_step"):
                nbytes = ((8.0 if what == "step" else 12.0) + 4.0 * 513 / 256) * B * S
                flops = n / 256.0 * (20.0 / 16.0) * (2 * 5.0 * 512 * 9 + 40.0 * 513)
                rec.update(hbm_gb=round(nbytes / 1e9, 4), tb_per_s=round(nbytes / ms / 1e9, 2), gflop=round(flops / 1e9, 2),
                           tflops=round(flops / ms / 1e9, 2))
            if what == "step":
                step_ms = ms
            if what == "fast_step":
                rec.update(momentum=a.momentum, over_plain_step=round(ms / step_ms, 3))
            if "call" in what:
                rec["us_per_iteration"] = round(ms * 1e3 / max(1, a.n_iter), 1)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
