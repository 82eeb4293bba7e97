#!/usr/bin/env python3
"""Teacher-forced forward and training step of a hard-duration model beside the soft one at the bench shape (B = 64, 100 tokens,
512 frames, bf16, one HIP graph each), timed in the same run: interleaved rounds of back-to-back replays, median and minimum.
With hard durations MAS sits on the decoder's critical path.
Usage: python tools/bench_hard_duration.py [--no-train]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import runtime, synth, train  # noqa: E402
from isp_tts_amd.acoustic import AcousticModel  # noqa: E402
from isp_tts_amd.config import AcousticDims  # noqa: E402
from isp_tts_amd.graph import GraphedForward  # noqa: E402

DEV = "cuda"
KEYS = ("text", "text_len", "mel", "mel_len", "pitch", "energy")


def model_for(soft: bool, trainable: bool):
    model = AcousticModel.init(AcousticDims().model_config(soft_duration=soft))
    model.load_state_dict(synth.make_state_dict(), strict=True)
    model = model.to(DEV).eval()
    return model if trainable else model.requires_grad_(False).set_compute_dtype(torch.bfloat16)


def interleaved(replays: dict, rounds: int = 9, inner: int = 10) -> dict:
    for fn in replays.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in replays}
    for _ in range(rounds):
        for k, fn in replays.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in times.items()}


if __name__ == "__main__":
    print(runtime.device_info())
    d = {k: v.to(DEV) for k, v in synth.make_inputs(64, 100, 512, variable=True).items()}
    fwd = {}
    for name, soft in (("soft", True), ("hard", False)):
        g = GraphedForward(model_for(soft, False), *(d[k] for k in KEYS), flow_noise=d["flow_x0"], flow_time=d["flow_t"])
        fwd[f"forward {name}"] = g.replay
    for k, (med, mn) in interleaved(fwd).items():
        print(f"{k:20s} median {med:7.3f} ms  min {mn:7.3f} ms")
    if "--no-train" not in sys.argv:
        steps = {}
        batch = {k: d[k] for k in (*KEYS, "flow_x0", "flow_t")}
        for name, soft in (("soft", True), ("hard", False)):
            model = model_for(soft, True)
            opt = train.FlatAdamW(list(model.parameters()), lr=2e-4, weight_decay=1e-2, grad_clip=1.0)
            opt.check_finite = False
            step = train.GraphedTrainStep(model, opt, batch, amp=True, warmup=2)
            steps[f"train step {name}"] = lambda step=step: step(**batch)
        for k, (med, mn) in interleaved(steps, rounds=7, inner=5).items():
            print(f"{k:20s} median {med:7.3f} ms  min {mn:7.3f} ms")
