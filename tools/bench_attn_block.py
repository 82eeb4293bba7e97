#!/usr/bin/env python3
"""Go / no-go of DESIGN 4.5b: ispk_attn_block_short_bf16 against the three launches it replaces (q/kv GEMM, attention, to_out GEMM
with mask + residual), each as a HIP graph of 20 blocks, interleaved (ROUNDS=15 rounds; the three-launch graph is captured twice:
the spread of two identical configurations).  Shapes: B x 100 for (dim 384, 6 heads) and (256, 4 heads) at B = 64 and B = 8, and the sizes around them.
Prints the medians, the spread and whether the outputs are equal.      python tools/bench_attn_block.py"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import runtime, synth
dev = "cuda"
ROUNDS, REP = int(os.environ.get("ROUNDS", 15)), 20
SHAPES = ((64, 100, 6), (64, 100, 4), (8, 100, 6), (8, 100, 4), (64, 128, 6), (64, 64, 6), (32, 100, 4), (16, 100, 4), (1, 100, 6), (1, 100, 4))
for B, N, H in SHAPES:
    D = 64 * H
    x = synth._normal(f"b/ab/x{B}{N}{D}", (B, N, D)).to(dev).to(torch.bfloat16)
    wqkv = synth._normal(f"b/ab/wq{D}", (D + 128, D), D ** -0.5).to(dev).to(torch.bfloat16)
    wo = synth._normal(f"b/ab/wo{D}", (D, D), D ** -0.5).to(dev).to(torch.bfloat16)
    resid = synth._normal(f"b/ab/r{B}{N}{D}", (B, N, D)).to(dev)
    slopes = torch.tensor(synth.alibi_default_slopes(H), device=dev)
    key_len = torch.tensor([N - (7 * i) % (N // 2) for i in range(B)], dtype=torch.int64, device=dev)
    mask = torch.arange(N, device=dev)[None, :] < key_len[:, None]
    wqkv_c, wo_c = runtime.chunk_k16(wqkv), runtime.chunk_k16(wo)

    def three():
        qkv = runtime.gemm(x, wqkv)
        o = runtime.alibi_mqa_attention(qkv, H, slopes, key_len)
        return runtime.gemm(o, wo, resid=resid, mask=mask, flags=runtime.EP_MASK_ACC, out_dtype=torch.float32), qkv

    def fused():
        return runtime.attn_block_short(x, wqkv_c, None, H, slopes, key_len, wo_c, resid, mask)

    def fused_qkv():     # finished q/kv rows as the input (the encoder's layer 0): against attention + to_out alone
        return runtime.attn_block_short(None, None, qkv_given, H, slopes, key_len, wo_c, resid, mask)

    def two():
        o = runtime.alibi_mqa_attention(qkv_given, H, slopes, key_len)
        return runtime.gemm(o, wo, resid=resid, mask=mask, flags=runtime.EP_MASK_ACC, out_dtype=torch.float32), qkv_given

    want, qkv_given = three()
    got, qkv_got = fused()
    same = torch.equal(got, want) and torch.equal(qkv_got, qkv_given) and torch.equal(fused_qkv()[0], want)
    configs = {"three launches": three, "three launches (again)": three, "one kernel": fused, "two launches (q/kv given)": two,
               "one kernel (q/kv given)": fused_qkv}
    graphs = {}
    for name, f in configs.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(REP):
                f()
        g.replay()
        torch.cuda.synchronize()
        graphs[name] = g
    res = {n: [] for n in graphs}
    for _ in range(ROUNDS):
        for name, g in graphs.items():
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / (5 * REP) * 1e3)
    med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
    spread = abs(med["three launches"] - med["three launches (again)"])
    gain = min(med["three launches"], med["three launches (again)"]) - med["one kernel"]
    print(f"B={B} N={N} dim={D}: outputs equal: {same}")
    for n, v in res.items():
        print(f"    {n:28s} median {med[n]:7.2f} us  (min {min(v):7.2f}, max {max(v):7.2f})")
    print(f"    gain {gain:6.2f} us, spread of identical configurations {spread:5.2f} us -> {'GO' if gain > 3 * spread and gain > 0 else 'NO-GO'}")
