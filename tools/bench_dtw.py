#!/usr/bin/env python3
"""Device time of ispk_dtw_f32 and ispk_mcd_dtw_f32 (csrc/dtw.hip) at B = 64 with 512 x 512, 512 x 640 and 1,723 x 1,723 frames:
HIP events around `--reps` back-to-back launches, median of `--rounds` rounds after a warm-up; per shape the time per launch, per
anti-diagonal step (N + M - 1 of them) and per cell, and the HBM bytes the launch moves against the algorithmic minimum.  One
JSON line per shape.

    python tools/bench_dtw.py [--batch 64] [--reps 10] [--rounds 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_dtw.py --kernel-only     # the kernels alone, 20 calls per shape
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import runtime  # noqa: E402
from isp_tts_amd.acoustic import create_dct  # noqa: E402

SHAPES = ((512, 512), (512, 640), (1723, 1723))


def operands(B, N, M):
    g = torch.Generator().manual_seed(N * 4096 + M)
    tgt = torch.randn(B, 80, M, generator=g) * 2.0 - 5.0
    idx = (torch.arange(N) * M) // N
    out = tgt[:, :, idx] + 0.5 * torch.randn(B, 80, N, generator=g)
    hz = lambda T: torch.where(torch.rand(B, T, generator=g) < 0.3, torch.zeros(B, T),   # noqa: E731
                               120.0 + 40.0 * torch.rand(B, T, generator=g))
    n_len, m_len = torch.full((B,), N, dtype=torch.int64), torch.full((B,), M, dtype=torch.int64)
    return [t.cuda() for t in (out, n_len, tgt, m_len, hz(N), hz(M))]


def timed(fn, reps, rounds):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true", help="20 calls of each entry per shape and nothing else")
    a = ap.parse_args()
    B = a.batch
    dct = create_dct(13, 80).cuda()
    for N, M in SHAPES:
        out, n_len, tgt, m_len, po, pt = operands(B, N, M)
        fused = lambda: runtime.mcd_dtw(out, n_len, tgt, m_len, dct, po, pt)   # noqa: E731
        cost = torch.empty((B, N, M), dtype=torch.float32, device=out.device)       # the plain entry's operand
        runtime.mcd_dtw(out, n_len, tgt, m_len, dct, po, pt, cost_out=cost)
        plain = lambda: runtime.dtw(cost, n_len, m_len)   # noqa: E731
        if a.kernel_only:
            for _ in range(20):
                fused()
                plain()
            torch.cuda.synchronize()
            continue
        cells, diags = B * N * M, N + M - 1
        res = {"B": B, "N": N, "M": M}
        for name, fn in (("dtw", plain), ("mcd_dtw", fused)):
            med, best = timed(fn, a.reps, a.rounds)
            res[f"{name}_us"] = round(med, 1)
            res[f"{name}_us_min"] = round(best, 1)
            res[f"{name}_ns_per_diagonal"] = round(med * 1e3 / diags, 1)
            res[f"{name}_ns_per_cell"] = round(med * 1e3 / cells, 4)
        # HBM bytes: the plain entry reads the cost, writes and re-reads its skewed copy, and writes 2 bits per cell + the
        # path; its minimum is the cost itself.  The fused entry reads both mels, writes and re-reads the skewed cost and
        # the cepstra; its minimum is the two mels.
        res["dtw_bytes"] = int(12.25 * cells + 4 * B * diags)
        res["dtw_bytes_min"] = 4 * cells
        res["mcd_dtw_bytes"] = int(8.25 * cells + 4 * B * (N + M) * (80 + 2 * 12))
        res["mcd_dtw_bytes_min"] = 4 * B * (N + M) * 80
        print(json.dumps(res))


if __name__ == "__main__":
    main()
