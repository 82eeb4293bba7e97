#!/usr/bin/env python3
"""Times of the word-level prosody pieces (isp_tts_amd.longform):
  * ispk_gain_envelope_f32 at 64 items x 131,072 samples with 128 tokens of 1,024 samples each and random gains, ramp 128,
    beside its traffic floor: every sample read once and written once (67 MB) over 6.3 TB/s (the memory rate the other sections
    of DESIGN.md use), the same launch with one token per item, and ATen's elementwise multiply of the same buffers;
  * ispk_infer_features_tokens_f32 beside ispk_infer_features_items_f32 at 64 x 128 tokens, soft and rounded;
  * a `Synthesizer` replay at the join's shape - 64 sentences of 32 tokens and 512 frames (131,072 samples) into 8 documents,
    HiFi-GAN V1, both conditioners, marks with 64 words - captured with `prosody` off (the chain as it was) and on, the rounds
    alternating between the two.  `--plain-only` times the chain without prosody alone and touches no name that a tree without
    the feature lacks: the same file then times an older checkout.
Device time from HIP events over `--reps` back-to-back calls after warm-up, median of `--rounds` rounds.  The two kernels are
timed twice: called eagerly, where the host's issue rate of about 13 us per Python-level call bounds the figure, and as
`--reps` calls captured into one HIP graph and replayed ("graphed"), which is what they cost inside a captured chain.  One JSON
line each.

    python tools/time_prosody.py [--reps 20] [--rounds 5] [--plain-only] [--skip-synthesizer]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import graph, longform, runtime, synth  # noqa: E402

MEMORY_TB_S = 6.3


def timed(fn, reps, rounds, every=False):
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
    return per if every else statistics.median(per)


def alternating(fns, reps, rounds):
    """Per-call device time of each of `fns`, the rounds alternating between them -> per fn all its rounds, in ms."""
    for fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    per = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per[k].append(e0.elapsed_time(e1) / reps)
    return per


def graphed(fn, reps, rounds):
    """Per-call device time of `reps` calls captured into one graph."""
    def many():
        for _ in range(reps):
            fn()
    g = graph.GraphedCall(many)
    return timed(g.replay, 1, rounds * 4) / reps


def us(ms):
    return round(ms * 1e3, 2)


def time_kernels(a, dev, g, note):
    B, S, L = 64, 131072, 128
    audio = torch.from_numpy(g.uniform(-0.5, 0.5, (B, S)).astype(np.float32)).to(dev)
    lens = torch.full((B,), S, dtype=torch.int64, device=dev)
    ends = torch.arange(1, L + 1, dtype=torch.int64, device=dev) * (S // L)
    marks = torch.stack([ends - S // L, ends], dim=1).repeat(B, 1, 1).contiguous()
    gain = torch.from_numpy(g.uniform(0.25, 2.0, (B, L)).astype(np.float32)).to(dev)
    out = torch.empty_like(audio)
    fn = lambda: runtime.gain_envelope(audio, lens, marks, gain, 128, out)      # noqa: E731
    t, tg = timed(fn, a.reps, a.rounds), graphed(fn, a.reps, a.rounds)
    nbytes = 8.0 * B * S
    # what the figure is made of: the same launch with ONE token over the whole item (no boundary, a one-probe search), and an
    # elementwise multiply of the same buffers by ATen (what this machine streams 67 MB in, no marks at all)
    one_marks = torch.tensor([0, S], dtype=torch.int64, device=dev).repeat(B, 1, 1).contiguous()
    one = graphed(lambda: runtime.gain_envelope(audio, lens, one_marks, gain[:, :1].contiguous(), 128, out), a.reps, a.rounds)
    mul = graphed(lambda: torch.mul(audio, 0.5, out=out), a.reps, a.rounds)
    print(json.dumps({"what": "gain_envelope", "B": B, "S": S, "L": L, "ramp": 128, "us_per_call": us(t), "graphed_us": us(tg),
                      "one_token_graphed_us": us(one), "aten_mul_graphed_us": us(mul),
                      "mb_moved": round(nbytes / 1e6, 2), "traffic_floor_us": round(nbytes / MEMORY_TB_S / 1e6, 2),
                      "tb_per_s_graphed": round(nbytes / tg / 1e9, 2), **note}), flush=True)
    L = 128
    pred = torch.from_numpy(g.standard_normal((B, L, 3)).astype(np.float32)).to(dev)
    items_c = longform.make_controls(B, duration_factor=list(g.uniform(0.8, 1.25, B)), device=dev)
    tokens_c = items_c[:, None, :].repeat(1, L, 1)
    for rnd in (False, True):
        tokens = lambda: runtime.infer_features_tokens(pred, None, None, None, tokens_c, round_duration=rnd)    # noqa: E731
        items = lambda: runtime.infer_features_items(pred, None, None, None, items_c, round_duration=rnd)       # noqa: E731
        print(json.dumps({"what": "infer_features_tokens" + (" (round)" if rnd else ""), "B": B, "L": L,
                          "us_per_batch": us(timed(tokens, a.reps, a.rounds)), "items_entry_us": us(timed(items, a.reps, a.rounds)),
                          "graphed_us": us(graphed(tokens, a.reps, a.rounds)), "items_entry_graphed_us": us(graphed(items, a.reps, a.rounds)),
                          **note}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--skip-synthesizer", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    g = np.random.default_rng(0)
    note = {"reps": a.reps, "rounds": a.rounds}
    if not a.plain_only:
        time_kernels(a, dev, g, note)
    if a.skip_synthesizer:
        return

    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    from isp_tts_amd.data import AudioConditioner
    from isp_tts_amd.hifigan import HifiGan
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    model = model.to(dev).requires_grad_(False)
    voc = HifiGan.from_state_dict(synth.make_hifigan_state_dict(), synth.HIFIGAN_DIMS["v1"]).to(dev).eval()
    B, L, M, D, W = 64, 32, 512, 8, 64
    S_out = B // D * M * 256
    inp = synth.make_inputs(B, L, M, variable=True, seed=5)
    syns = []
    for extra in ({},) if a.plain_only else ({}, {"prosody": True, "ramp": 128}):
        syn = longform.Synthesizer(model, voc, batch=B, tokens=L, frames=M, docs=D, doc_samples=S_out, fade=64,
                                   item_conditioner=AudioConditioner(22050, target_lufs=None),
                                   doc_conditioner=AudioConditioner(22050), marks=True, words=W, **extra)
        for k, v in (("text", inp["text"]), ("text_len", inp["text_len"]), ("flow_noise", inp["flow_x0"])):
            syn.static[k].copy_(v.to(dev))
        syn.static["doc"].copy_(torch.arange(B, device=dev) % D)
        syn.static["word_id"].copy_((torch.arange(L, device=dev) // 2).repeat(B, 1))
        if extra:
            syn.static["gain"].copy_(torch.from_numpy(g.uniform(0.5, 1.5, (B, L)).astype(np.float32)).to(dev))
        syns.append(syn)
    reps, rounds = max(1, a.reps // 4), 2 * a.rounds + 1
    per = alternating([s._graph.replay for s in syns], reps, rounds)
    row = {"what": "Synthesizer replay, prosody off" + ("" if a.plain_only else " / on, rounds alternating"), "B": B, "L": L, "M": M,
           "D": D, "S_out": S_out, "words": W, "prosody_off_us": us(statistics.median(per[0])),
           "prosody_off_range_us": [us(min(per[0])), us(max(per[0]))]}
    if not a.plain_only:
        row.update(prosody_on_us=us(statistics.median(per[1])), prosody_on_range_us=[us(min(per[1])), us(max(per[1]))],
                   difference_us=us(statistics.median(per[1]) - statistics.median(per[0])))
    print(json.dumps({**row, "reps": reps, "rounds": rounds}), flush=True)


if __name__ == "__main__":
    main()
