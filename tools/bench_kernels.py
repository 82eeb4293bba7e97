#!/usr/bin/env python3
"""Micro-benchmark of the hot kernels at the BASELINE config-3 shapes (B=64: 32768 decoder rows, 6400 encoder rows).
HIP-event timing, interleaved rounds, median.  Usage: python tools/bench_kernels.py [f32|bf16] [--rows 32768]
`python tools/bench_kernels.py adaptor`: the temporal adaptor's regulators and averagers instead, hard durations beside soft, and
the speaker-embedding add with its table gradient, at B=64, L=100, M=512, D=384, each with its traffic floor at the 6.3 TB/s a float4 copy reaches on the MI355X.
`python tools/bench_kernels.py hifigan [bf16]`: the HiFi-GAN convolution kernels (csrc/hifigan.hip) at the V1 stage shapes of the
B=64 x 512-frame batch."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isp_tts_amd import runtime, synth  # noqa: E402

dt = torch.bfloat16 if (len(sys.argv) > 1 and sys.argv[1] == "bf16") else torch.float32
R = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 32768
dev = "cuda"


def time_it(fn, rounds=7, inner=20):
    """Median over rounds of (time of `inner` back-to-back launches) / inner: excludes the ~15 us idle-launch +
    event floor that a single timed launch carries."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def adaptor_cases():
    """Hard-duration kernels (csrc/hard_duration.hip) beside the soft ones they stand in for, same run, same inputs."""
    B, L, M, D = 64, 100, 512, 384
    inp = synth.make_inputs(B, L, M, variable=True)
    tl, ml = inp["text_len"], inp["mel_len"]
    dur = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):                                   # integer durations over the valid tokens that sum to mel_len, as MAS gives
        n, m = int(tl[b]), int(ml[b])
        dur[b, :n] = m // n
        dur[b, :m - (m // n) * n] += 1
    x = synth._normal("b/adaptor/x", (B, L, D)).to(dev)
    d_out = synth._normal("b/adaptor/dout", (B, M, D)).to(dev)
    attn = torch.softmax(synth._normal("b/adaptor/attn", (B, M, L)), dim=-1).to(dev)
    pred = synth._normal("b/adaptor/pred", (B, L, 3)).to(dev)
    dur_d, dur_f, tl_d = dur.to(dev), dur.float().to(dev), tl.to(dev)
    pitch, energy = inp["pitch"].to(dev), inp["energy"].to(dev)
    rows = 4 * B * D * (M + L)
    S = 1307                                             # the published multi-speaker checkpoint's table
    table = synth._normal("b/adaptor/speakers", (S, D), 0.3).to(dev)
    d_table = torch.empty_like(table)
    ids = (torch.arange(B).view(B, 1) * 20 % S).to(dev)
    ids4 = ids % 4
    d_x = d_out[:, :L].contiguous()
    return [
        ("hard regulate (int64 durations)", lambda: runtime.hard_regulate(x, dur_d, M, max_len=M), rows),
        ("hard regulate (fp32 durations)", lambda: runtime.hard_regulate(x, dur_f, M), rows),
        ("soft regulate fp32 MFMA", lambda: runtime.length_regulate(x, dur_d, attn, M, max_len=M), rows + 4 * B * M * L),
        ("soft regulate split bf16", lambda: runtime.length_regulate(x, dur_d, attn, M, max_len=M, split_bf16=True), rows + 4 * B * M * L),
        ("soft regulate, path from durations", lambda: runtime.length_regulate(x, dur_f, None, M, enc_len=tl_d), rows),
        ("hard regulate backward", lambda: runtime.hard_regulate_bwd(d_out, dur_d, M), rows),
        ("soft regulate backward (A^T dOut)", lambda: runtime.gemm_tn_batched(attn, d_out), rows + 4 * B * M * L),
        ("hard average", lambda: runtime.hard_average(pitch, energy, dur_d, tl_d), 8 * B * M + 20 * B * L),
        ("soft average", lambda: runtime.soft_average(attn, pitch, energy, dur_d, tl_d), 4 * B * M * L + 8 * B * M + 20 * B * L),
        ("infer features, rounded", lambda: runtime.infer_features(pred, None, None, None, round_duration=True), 24 * B * L),
        ("infer features", lambda: runtime.infer_features(pred, None, None, None), 24 * B * L),
        ("add speaker, out of place", lambda: runtime.add_speaker(x, table, ids), 8 * B * L * D),
        ("add speaker, in place", lambda: runtime.add_speaker_(x, table, ids), 8 * B * L * D),
        (f"speaker table gradient, S={S}", lambda: runtime.speaker_grad(d_x, ids, S, tl_d, out=d_table), 4 * B * L * D + 4 * S * D),
        ("speaker table gradient, S=4", lambda: runtime.speaker_grad(d_x, ids4, 4, tl_d, out=d_table[:4]), 4 * B * L * D),
    ]


if "adaptor" in sys.argv:
    print("adaptor kernels, B=64 L=100 M=512 D=384 (floor: bytes / 6.3 TB/s)")
    for name, fn, nbytes in adaptor_cases():
        med, mn = time_it(fn)
        print(f"{name:36s} median {med:7.1f} us  min {mn:7.1f} us  {nbytes / 1e6:7.2f} MB  floor {nbytes / 6.3e6:6.2f} us  {nbytes / med / 1e3:7.1f} GB/s")
    sys.exit(0)

def hifigan_cases():
    """One dilated convolution and the transposed convolution of every V1 stage, plus the output layer, at B=64 x 512 frames."""
    B, T, C = 64, 512, 512
    cases = []
    for u, ku, (k, d) in zip((8, 8, 2, 2), (16, 16, 4, 4), ((7, 3), (7, 3), (11, 5), (11, 5))):
        x = synth._normal(f"b/hfg/x{C}", (B * T, C)).to(dev)
        wu = synth._normal(f"b/hfg/up{C}", (ku, C // 2, C), (C * ku / u) ** -0.5).to(dev).to(dt)
        up = torch.empty((B * T * u, C // 2), device=dev)
        cases.append((f"upsample {C}->{C // 2} k={ku} u={u} T={T}", lambda x=x, wu=wu, up=up, T=T, ku=ku, u=u:
                      runtime.hifigan_upsample(x, T, wu, None, ku, u, out=up), 2 * B * T * C * (C // 2) * ku,
                      4 * B * T * (C + u * C // 2)))
        T, C = T * u, C // 2
        wc = synth._normal(f"b/hfg/w{C}", (k, C, C), (C * k) ** -0.5).to(dev).to(dt)
        y = torch.empty_like(up)
        cases.append((f"conv {C} k={k} d={d} T={T} +resid", lambda up=up, wc=wc, y=y, T=T, k=k, d=d:
                      runtime.hifigan_conv(up, T, wc, None, k, d, 0.1, resid=up, out=y), 2 * B * T * C * C * k, 12 * B * T * C))
        del x
    wp, bp = synth._normal("b/hfg/post", (7, C), 0.1).to(dev), torch.zeros(1, device=dev)
    audio = torch.empty((B, T), device=dev)
    cases.append((f"post {C}->1 T={T}", lambda: runtime.hifigan_post(y, T, wp, bp, audio), 14 * B * T * C, 4 * B * T * (C + 1)))
    return cases


if "hifigan" in sys.argv:
    dt = torch.bfloat16 if "bf16" in sys.argv else torch.float32
    print(f"HiFi-GAN V1 kernels, B=64 x 512 frames, {dt}")
    for name, fn, flops, nbytes in hifigan_cases():
        med, mn = time_it(fn, rounds=5, inner=3)
        print(f"{name:40s} median {med:9.1f} us  min {mn:9.1f} us  {flops / med / 1e6:7.1f} TFLOP/s  {nbytes / med / 1e3:7.1f} GB/s")
    sys.exit(0)

x384 = synth._normal("b/x", (R, 384)).to(dev).to(dt)
x1536 = synth._normal("b/x2", (R, 1536)).to(dev).to(dt)
resid = synth._normal("b/r", (R, 384)).to(dev)
mask = torch.ones(R, dtype=torch.bool, device=dev)
w = {n: synth._normal(f"b/w{n}", s, s[1] ** -0.5).to(dev).to(dt) for n, s in
     {"qkv": (512, 384), "o": (384, 384), "f1": (1536, 384), "f2": (384, 1536)}.items()}
odt = dt
cases = [
    ("qkv   [R,384]x[512,384]", lambda: runtime.gemm(x384, w["qkv"]), 2 * R * 512 * 384, R * (384 + 512) * x384.element_size()),
    ("out   [R,384]x[384,384]+res", lambda: runtime.gemm(x384, w["o"], resid=resid, mask=mask, flags=runtime.EP_MASK_ACC,
                                                         out_dtype=torch.float32), 2 * R * 384 * 384, R * 384 * (x384.element_size() + 8)),
    ("ffn1  [R,384]x[1536,384]+gelu", lambda: runtime.gemm(x384, w["f1"], flags=runtime.EP_GELU), 2 * R * 1536 * 384,
     R * (384 + 1536) * x384.element_size()),
    ("ffn2  [R,1536]x[384,1536]+res", lambda: runtime.gemm(x1536, w["f2"], resid=resid, mask=mask, flags=runtime.EP_MASK_OUT,
                                                           out_dtype=torch.float32), 2 * R * 384 * 1536,
     R * (1536 * x384.element_size() + 384 * 8)),
    ("layernorm [R,384]", lambda: runtime.layernorm(resid, None, None, out_dtype=dt), 0, R * 384 * (4 + x384.element_size())),
]
B, N = R // 512, 512
qkv = synth._normal("b/qkv", (B, N, 512)).to(dev).to(dt)
slopes = torch.tensor(synth.alibi_default_slopes(6), device=dev)
cases.append((f"attn  B={B} N={N} H=6", lambda: runtime.alibi_mqa_attention(qkv, 6, slopes, None), 256 * B * N * N * 6,
              B * N * (2 * 384 + 128) * qkv.element_size()))
print(f"dtype={dt} rows={R}")
for name, fn, flops, nbytes in cases:
    med, mn = time_it(fn)
    print(f"{name:34s} median {med:8.1f} us  min {mn:8.1f} us  {flops / med / 1e6:8.1f} TFLOP/s  {nbytes / med / 1e3:8.1f} GB/s")
if dt == torch.bfloat16:
    med, mn = time_it(lambda: runtime.ffn_fused(x384, w["f1"], w["f2"], resid=resid, mask=mask, flags=runtime.EP_MASK_OUT))
    fl = 4 * R * 384 * 1536
    print(f"{'fused ffn [R,384]->1536->384+res':34s} median {med:8.1f} us  min {mn:8.1f} us  {fl / med / 1e6:8.1f} TFLOP/s")
