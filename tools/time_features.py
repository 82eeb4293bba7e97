#!/usr/bin/env python3
"""Time of the feature extractor (data.AcousticFeatures, one ispk_audio_features_f32 launch) at the bench shape (B = 64
utterances of 131,072 samples = 512 frames), and of the captured AMP training step from audio (GraphedTrainStep(features=))
against the same step from precomputed features.  Device time from HIP events over `--reps` back-to-back calls, median of
`--rounds` rounds; one JSON line.

    python tools/time_features.py [--batch 64] [--samples 131072] [--reps 50] [--rounds 5] [--no-step]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_features.py --no-step     # the kernel alone
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import synth, train  # noqa: E402
from isp_tts_amd.acoustic import AcousticModel  # noqa: E402
from isp_tts_amd.config import AcousticDims  # noqa: E402
from isp_tts_amd.data import AcousticFeatures, collate_audio  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="only the extractor")
    a = ap.parse_args()
    kinds = synth.CLIP_KINDS
    waves = [synth.make_clip(kinds[i % len(kinds)], a.samples, 0.5, seed=i) for i in range(a.batch)]
    audio, lens = collate_audio(waves)
    audio, lens = audio.cuda(), lens.cuda()
    feats = AcousticFeatures(pitch_mean=166.6177, pitch_std=62.5423)
    out = feats(audio, lens)
    torch.cuda.synchronize()
    res = {"batch": a.batch, "samples": a.samples, "frames": int(out["mel"].shape[2]),
           "features_ms": timed(lambda: feats(audio, lens, out=out), a.reps, a.rounds)}
    if not a.no_step:
        inp = {k: v.cuda() for k, v in synth.make_inputs(a.batch, 100, res["frames"], variable=True).items()}
        common = {k: inp[k] for k in ("text", "text_len", "flow_x0", "flow_t")}
        sd = synth.make_state_dict()
        for name, batch, f in (("step_from_features_ms", dict(common, **{k: out[k] for k in out}), None),
                               ("step_from_audio_ms", dict(common, audio=audio, audio_len=lens), feats)):
            model = AcousticModel.init(AcousticDims().model_config())
            model.load_state_dict(sd, strict=True)
            model = model.to("cuda").train()
            opt = train.FlatAdamW(model.parameters(), lr=2e-4, weight_decay=1e-2, grad_clip=1.0)
            step = train.GraphedTrainStep(model, opt, batch, amp=True, features=f)
            for _ in range(3):
                step()
            res[name] = timed(step, 20, a.rounds)
            step.close()
            del step, opt, model
            torch.cuda.empty_cache()
        res["features_cost_in_graph_ms"] = res["step_from_audio_ms"] - res["step_from_features_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
