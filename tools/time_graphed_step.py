#!/usr/bin/env python3
"""Time of one replay of the captured AMP training step (train.GraphedTrainStep) at the bench shape (B = 64, 100 tokens, 512
frames), with and without `evaluator=AcousticModelEvaluator(model)`, and of the evaluator's own launch pair on that step's
outputs.  Device time per replay from HIP events over `--reps` back-to-back replays, median of `--rounds` rounds; one JSON line.
`--speakers`: instead, the plain model's step beside that of a 4-speaker model with `speaker_in_forward` on (one more static
input, two more launches, one more 2-D tensor in the arena), both captured first and then timed in interleaved rounds.

    python tools/time_graphed_step.py [--batch 64] [--reps 20] [--rounds 5] [--speakers]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_graphed_step.py --kernel-only   # the metric kernels alone
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import synth, train  # noqa: E402
from isp_tts_amd.acoustic import AcousticModel, AcousticModelEvaluator  # noqa: E402
from isp_tts_amd.config import AcousticDims  # noqa: E402


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


def speakers_main(a):
    d = {k: v.to("cuda") for k, v in synth.make_inputs(a.batch, 100, 512, variable=True).items()}
    batch = {k: d[k] for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy", "flow_x0", "flow_t")}
    sd = synth.make_state_dict()
    steps = {}
    for name, speakers in (("step_ms", 0), ("step_speakers_ms", 4)):
        model = AcousticModel.init(dict(AcousticDims().model_config(), num_speakers=speakers), speaker_in_forward=True)
        if speakers:
            sd = dict(sd, **{"speaker_embedding.weight": synth.make_speaker_table(speakers)})
            batch = dict(batch, speaker=(torch.arange(a.batch, device="cuda") % speakers).view(-1, 1))
        model.load_state_dict(sd, strict=True)
        model = model.to("cuda").train()
        opt = train.FlatAdamW(model.parameters(), lr=2e-4, weight_decay=1e-2, grad_clip=1.0)
        steps[name] = train.GraphedTrainStep(model, opt, batch, amp=True)
        for _ in range(3):
            steps[name]()
    per = {name: [] for name in steps}
    for _ in range(a.rounds):                        # interleaved: both models see the same clocks and the same neighbours
        for name, step in steps.items():
            per[name].append(timed(step, a.reps, 1))
    res = {"batch": a.batch, "text_len": 100, "mel_len": 512, "rounds": a.rounds, "reps": a.reps}
    res.update({name: statistics.median(v) for name, v in per.items()})
    res["speakers_cost_ms"] = res["step_speakers_ms"] - res["step_ms"]
    print(json.dumps(res))
    for step in steps.values():
        step.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="only 100 evaluator calls on synthetic bench-shape operands")
    ap.add_argument("--speakers", action="store_true", help="the plain step beside a 4-speaker model's with speaker_in_forward on")
    a = ap.parse_args()
    if a.speakers:
        return speakers_main(a)
    if a.kernel_only:
        g = torch.Generator().manual_seed(0)
        mel_len = torch.randint(64, 513, (a.batch,), generator=g)
        mel_len[0] = 512
        inputs = {"mel": torch.randn(a.batch, 80, 512, generator=g).cuda(), "mel_len": mel_len.cuda(),
                  "text_len": torch.randint(25, 101, (a.batch,), generator=g).cuda()}
        outputs = {"mel": torch.randn(a.batch, 80, 512, generator=g).cuda(),
                   "aligner_output": {"attn_soft": torch.softmax(torch.randn(a.batch, 512, 100, generator=g), -1).cuda()}}
        ev = AcousticModelEvaluator()
        print(json.dumps({"evaluator_eager_ms": timed(lambda: ev(inputs, outputs), 100, a.rounds)}))
        return
    d = {k: v.to("cuda") for k, v in synth.make_inputs(a.batch, 100, 512, variable=True).items()}
    batch = {k: d[k] for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy", "flow_x0", "flow_t")}
    sd = synth.make_state_dict()
    res = {"batch": a.batch, "text_len": 100, "mel_len": 512}
    for name, with_eval in (("step_ms", False), ("step_with_evaluator_ms", True)):
        model = AcousticModel.init(AcousticDims().model_config())
        model.load_state_dict(sd, strict=True)
        model = model.to("cuda").train()
        opt = train.FlatAdamW(model.parameters(), lr=2e-4, weight_decay=1e-2, grad_clip=1.0)
        ev = AcousticModelEvaluator(model) if with_eval else None
        step = train.GraphedTrainStep(model, opt, batch, amp=True, evaluator=ev)
        for _ in range(3):
            step()
        res[name] = timed(step, a.reps, a.rounds)
        if with_eval:
            inputs = {k: batch[k] for k in ("mel", "mel_len", "text_len")}
            res["evaluator_eager_ms"] = timed(lambda: ev(inputs, step.outputs), 50, a.rounds)
        step.close()
        del step, opt, model
        torch.cuda.empty_cache()
    res["evaluator_cost_in_graph_ms"] = res["step_with_evaluator_ms"] - res["step_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
