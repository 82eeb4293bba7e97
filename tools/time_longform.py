#!/usr/bin/env python3
"""Times of the long-form pieces (isp_tts_amd.longform):
  * ispk_infer_features_items_f32 at 64 x 100 tokens (soft and rounded), beside ispk_infer_features_f32 on the same rows;
  * the ispk_join_plan + ispk_join_f32 pair at 64 items x 131,072 samples into 8 documents (pauses, crossfades and fades mixed),
    beside the pair's traffic floor: every item sample read once and every document sample written once, over 6.3 TB/s (the
    memory rate the other sections of DESIGN.md use);
  * a `Synthesizer` replay (text -> PCM16 documents, HiFi-GAN V1) against the same chain captured without the join: 16 sentences
    of 32 tokens and 128 frames into 4 documents;
  * the speech marks: ispk_speech_marks alone at 64 items of 32 and of 4,096 tokens with 64 words each, soft and
    hard, with every optional input; and a `Synthesizer` replay at the join's shape - 64 sentences of 32 tokens and 512 frames
    (131,072 samples) into 8 documents - captured with `marks` off (the chain as it was) and on (words = 64).
Device time from HIP events over `--reps` back-to-back calls after warm-up, median of `--rounds` rounds.  The two small
pieces are timed twice: called eagerly, where the host's issue rate of about 13 us per Python-level call bounds the figure, and
as `--reps` calls captured into one HIP graph and replayed ("graphed"), which is what they cost inside a captured chain.  One
JSON line each.

    python tools/time_longform.py [--reps 20] [--rounds 5] [--skip-synthesizer] [--skip-marks]
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


def alternating(fns, reps, rounds):
    """Per-call device time of each of `fns`, the rounds alternating between them (a, b, a, b, ...), so that drift and other
    people's work on the machine fall on both alike -> per fn all its rounds, in ms."""
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


def time_marks(a, dev, g, note):
    """ispk_speech_marks alone: 64 items with bounds, the join group, document bounds and 64 words."""
    B, D, W, hop = 64, 8, 64, 256
    for L in (32, 4096):
        d = torch.from_numpy(g.uniform(0.0, 4.0, (B, L)).astype(np.float32)).to(dev)
        tl = torch.from_numpy(g.integers(L // 2, L + 1, B)).to(dev)
        S = int(hop * 4 * L)
        al = torch.from_numpy(g.integers(S // 4, S // 2, B)).to(dev)
        bounds = torch.stack([al // 16, al - al // 16], dim=1).contiguous()
        doc = torch.arange(B, device=dev) % D
        off = (torch.arange(B, device=dev) // D) * (S // 2)
        doc_len = torch.full((D,), B // D * (S // 2), dtype=torch.int64, device=dev)
        doc_bounds = torch.stack([doc_len // 64, doc_len - doc_len // 64], dim=1).contiguous()
        wid = (torch.arange(L, device=dev) * W // L).repeat(B, 1)
        out = longform.marks_outputs(B, L, W, dev)
        row = {"what": "speech_marks", "B": B, "L": L, "words": W, "D": D}
        for hard in (False, True):
            fn = lambda: runtime.speech_marks(d, tl, al, out["token_marks"], out["word_marks"], hop, S, hard, bounds, off, doc,   # noqa: E731
                                              doc_len, doc_bounds, wid)
            name = "hard" if hard else "soft"
            row[name + "_us"], row[name + "_graphed_us"] = round(timed(fn, a.reps, a.rounds) * 1e3, 2), round(graphed(fn, a.reps, a.rounds) * 1e3, 2)
        print(json.dumps({**row, **note}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-synthesizer", action="store_true")
    ap.add_argument("--skip-marks", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    g = np.random.default_rng(0)
    note = {"reps": a.reps, "rounds": a.rounds}

    # ---- the items kernel
    B, L = 64, 100
    pred = torch.from_numpy(g.standard_normal((B, L, 3)).astype(np.float32)).to(dev)
    controls = longform.make_controls(B, duration_factor=list(g.uniform(0.8, 1.25, B)), device=dev)
    for rnd in (False, True):
        items = lambda: runtime.infer_features_items(pred, None, None, None, controls, round_duration=rnd)      # noqa: E731
        scalar = lambda: runtime.infer_features(pred, None, None, None, 1.1, round_duration=rnd)                # noqa: E731
        t_i, t_s = timed(items, a.reps, a.rounds), timed(scalar, a.reps, a.rounds)
        g_i, g_s = graphed(items, a.reps, a.rounds), graphed(scalar, a.reps, a.rounds)
        print(json.dumps({"what": "infer_features_items" + (" (round)" if rnd else ""), "B": B, "L": L,
                          "us_per_batch": round(t_i * 1e3, 2), "scalar_entry_us": round(t_s * 1e3, 2),
                          "graphed_us": round(g_i * 1e3, 2), "scalar_entry_graphed_us": round(g_s * 1e3, 2), **note}), flush=True)

    # ---- plan + join
    B, S, D = 64, 131072, 8
    audio = torch.from_numpy(g.uniform(-0.5, 0.5, (B, S)).astype(np.float32)).to(dev)
    lens = torch.from_numpy(g.integers(S // 2, S + 1, B)).to(dev)
    doc = torch.arange(B, device=dev) % D
    pos = torch.from_numpy(g.permutation(B)).to(dev)
    pause = torch.from_numpy(g.choice([0, 4410, -2205, 11025], B)).to(dev)
    S_out = int(lens.sum().item() // D * 5 // 4)
    out = longform.join_outputs(D, S_out, B, dev)
    both = lambda: longform.join(audio, lens, doc, pos, pause, num_docs=D, out_samples=S_out, fade=64, out=out)   # noqa: E731
    plan = lambda: runtime.join_plan(lens, doc, pos, pause, None, out["plan"], out["item_offset"], out["item_len"],   # noqa: E731
                                     out["audio_len"], out["wanted_len"], S, S_out, 64)
    t_both, t_plan = timed(both, a.reps, a.rounds), timed(plan, a.reps, a.rounds)
    g_both, g_plan = graphed(both, a.reps, a.rounds), graphed(plan, a.reps, a.rounds)
    kept = int(out["item_len"].sum().item())
    nbytes = 4.0 * (kept + D * S_out)
    print(json.dumps({"what": "join_plan + join", "B": B, "S": S, "D": D, "S_out": S_out, "fade": 64, "us_per_call": round(t_both * 1e3, 2),
                      "plan_alone_us": round(t_plan * 1e3, 2), "graphed_us": round(g_both * 1e3, 2),
                      "plan_alone_graphed_us": round(g_plan * 1e3, 2), "mb_moved": round(nbytes / 1e6, 2),
                      "traffic_floor_us": round(nbytes / MEMORY_TB_S / 1e6, 2),
                      "tb_per_s_graphed": round(nbytes / g_both / 1e9, 2), "docs_cut": int((out["wanted_len"] > S_out).sum().item()), **note}),
          flush=True)
    if not a.skip_marks:
        time_marks(a, dev, g, note)
    if a.skip_synthesizer:
        return

    # ---- a Synthesizer replay against the same chain without the join
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    from isp_tts_amd.data import AudioConditioner, to_pcm16
    from isp_tts_amd.hifigan import HifiGan
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    model = model.to(dev).requires_grad_(False)
    voc = HifiGan.from_state_dict(synth.make_hifigan_state_dict(), synth.HIFIGAN_DIMS["v1"]).to(dev).eval()
    B, L, M, D = 16, 32, 128, 4
    S_out = B // D * M * 256
    syn = longform.Synthesizer(model, voc, batch=B, tokens=L, frames=M, docs=D, doc_samples=S_out,
                               item_conditioner=AudioConditioner(22050, target_lufs=None), doc_conditioner=AudioConditioner(22050), fade=64)
    inp = synth.make_inputs(B, L, M, variable=True, seed=5)
    for k, v in (("text", inp["text"]), ("text_len", inp["text_len"]), ("flow_noise", inp["flow_x0"])):
        syn.static[k].copy_(v.to(dev))
    syn.static["doc"].copy_(torch.arange(B, device=dev) % D)
    s = syn.static
    cond = AudioConditioner(22050)
    wav = voc.empty_outputs(B, M, dev)
    c_out = cond.empty_outputs(B, wav[0].shape[1], dev)
    pcm = torch.empty(wav[0].shape, dtype=torch.int16, device=dev)

    def per_item_chain():      # the chain the tree had before: per-item conditioning, no documents
        with torch.no_grad():
            mel, ao = model.infer(s["text"], text_lengths=s["text_len"], steps=4, flow_noise=s["flow_noise"], max_dec_len=M,
                                  controls=s["controls"])
            audio_, n_ = voc(mel, ao.dec_lengths, out=wav)
            r = cond(audio_, n_, out=c_out)
            return to_pcm16(r["audio"], r["audio_len"], out=pcm)

    plain = graph.GraphedCall(per_item_chain)
    t_syn, t_plain = timed(syn._graph.replay, max(1, a.reps // 4), a.rounds), timed(plain.replay, max(1, a.reps // 4), a.rounds)
    print(json.dumps({"what": "Synthesizer replay", "B": B, "L": L, "M": M, "D": D, "S_out": S_out, "us_per_replay": round(t_syn * 1e3, 1),
                      "chain_without_join_us": round(t_plain * 1e3, 1), "reps": max(1, a.reps // 4), "rounds": a.rounds}), flush=True)
    if a.skip_marks:
        return

    # ---- the same chain at the join's shape (64 x 131,072 samples into 8 documents), marks off and on
    del syn, plain
    B, L, M, D, W = 64, 32, 512, 8, 64
    S_out = B // D * M * 256
    inp = synth.make_inputs(B, L, M, variable=True, seed=5)
    syns = {}
    for marks in (False, True):
        syn = syns[marks] = longform.Synthesizer(model, voc, batch=B, tokens=L, frames=M, docs=D, doc_samples=S_out, fade=64,
                                                 item_conditioner=AudioConditioner(22050, target_lufs=None),
                                                 doc_conditioner=AudioConditioner(22050), marks=marks, words=W if marks else 0)
        for k, v in (("text", inp["text"]), ("text_len", inp["text_len"]), ("flow_noise", inp["flow_x0"])):
            syn.static[k].copy_(v.to(dev))
        syn.static["doc"].copy_(torch.arange(B, device=dev) % D)
        if marks:
            syn.static["word_id"].copy_((torch.arange(L, device=dev) // 2).repeat(B, 1))
    reps, rounds = max(1, a.reps // 4), 2 * a.rounds + 1
    off, on = alternating([syns[False]._graph.replay, syns[True]._graph.replay], reps, rounds)
    us = lambda ms: round(ms * 1e3, 1)      # noqa: E731
    print(json.dumps({"what": "Synthesizer replay, marks off / on, rounds alternating", "B": B, "L": L, "M": M, "D": D, "S_out": S_out,
                      "words": W, "marks_off_us": us(statistics.median(off)), "marks_on_us": us(statistics.median(on)),
                      "difference_us": us(statistics.median(on) - statistics.median(off)),
                      "marks_off_range_us": [us(min(off)), us(max(off))], "marks_on_range_us": [us(min(on)), us(max(on))],
                      "reps": reps, "rounds": rounds}), flush=True)


if __name__ == "__main__":
    main()
