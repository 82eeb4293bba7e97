#!/usr/bin/env python3
"""Same-box A/B of the graphed bf16 forward (B = 64 x 100 x 512, or BATCH=8) over the hand-off switches of DESIGN 4.2b and the
short attention block of DESIGN 4.5b per stack (`Attention.short_block` of the text encoder's, the embedding stack's and the flow
predictor's layers): all on (captured twice: the spread of two identical configurations), each one off, all off; every graph in
one process, interleaved rounds (ROUNDS=15).  ONLY=short_block restricts the switches to those whose name starts with it."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import synth
from isp_tts_amd.acoustic import AcousticModel
from isp_tts_amd.config import AcousticDims
from isp_tts_amd.graph import GraphedForward
model = AcousticModel.init(AcousticDims().model_config()).eval()
model.load_state_dict(synth.make_state_dict(), strict=True)
model = model.to("cuda").requires_grad_(False)
model.set_compute_dtype(torch.bfloat16)
d = {k: v.to("cuda") for k, v in synth.make_inputs(int(os.environ.get("BATCH", 64)), 100, 512).items()}


def attr(owner, name):
    return lambda on: setattr(owner, name, on)


def short_block(stack):
    return lambda on: [setattr(layer.attention, "short_block", on) for layer in stack.layers]


ta = model.temporal_adaptor
switches = {"token_qkv_table": attr(model, "token_qkv_table"), "hand_qkv": attr(ta.length_regulator, "hand_qkv"),
            "short_block encoder": short_block(model.encoder), "short_block embedding": short_block(ta.embedding.transformer),
            "short_block predictor": short_block(ta.predictor.transformer)}
switches = {k: v for k, v in switches.items() if k.startswith(os.environ.get("ONLY", ""))}
configs = {"all on": {}, "all on (again)": {}, "all off": {k: False for k in switches}}
for k in switches:
    configs[f"{k} off"] = {k: False}
graphs = {}
for name, off in configs.items():
    for k, set_to in switches.items():
        set_to(off.get(k, True))
    graphs[name] = GraphedForward(model, d["text"], d["text_len"], d["mel"], d["mel_len"], d["pitch"], d["energy"], d["flow_x0"], d["flow_t"])
res = {n: [] for n in graphs}
ROUNDS = int(os.environ.get("ROUNDS", 15))
for rnd in range(ROUNDS):
    for name, g in graphs.items():
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(30):
            g.replay()
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t0) / 30 * 1e3)
for set_to in switches.values():
    set_to(True)
for name, v in res.items():
    v = sorted(v)
    print(f"{name:28s}: median {v[len(v) // 2]:.4f} ms, min {v[0]:.4f} ms, max {v[-1]:.4f} ms")
