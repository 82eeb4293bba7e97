"""GPU: the iSTFTNet generator (isp_tts_amd.istftnet.IstftNet: csrc/istftnet.hip behind the HiFi-GAN stages).

Kernel level: ispk_istftnet_head_f32 alone against float64 (tests/istftnet_reference.py, whose torch.istft
tests/test_istftnet_host.py checks against a literal sum) under a per-sample a-priori bound, at the frame-tile edges
(TF = runtime.ISTFTNET_TILE_FRAMES), with NaN in every padded row; and on an input whose frames are exactly "on" (magnitude
exp(0) = 1 on the DC bin, phase 0) or "off" (exp(-200) = 0), where the waveform is a closed form of the window alone and the
reflection pad and the per-utterance envelope show to the ulp.

Whole model against the float64 module run utterance by utterance.  Bounds, per utterance, over its samples m < hop mel_len
(the project's vocoder bounds):
  fp32   max |audio - ref64| <= 1e-4 x max |ref64|
  bf16   max |audio - ref64| <= BF16_FACTOR x max |ref_bf16 - ref64|, ref_bf16 = the float64 module with the input and the
         weight of every convolution but conv_post rounded to bf16 (istftnet_reference.forward_bf16_operands)
and exactly 0 at and past hop mel_len.  Measured on gfx950 (one run): fp32 worst err / peak 2.4e-6 (c8c8i), 1.7e-6 (odd),
1.8e-6 (n20); bf16 worst err / bf16-operand error 1.20 (c8c8i), 1.18 (odd), 1.00 (n20).  Kernel alone: max |err| 6.7e-7
under bounds of 1.6e-4 (C = 32) to 5.8e-3 (C = 256), at no sample more than 1.1e-3 of its bound; the exact input: worst
0.89 ulp (16 / 4), 0.33 (8 / 2), 1.28 (20 / 5).

Then the padding semantics, determinism, graph capture (alone, and behind AcousticModel.infer with the conditioner and the
PCM16 export), SynthesisEvaluator.score_infer, Denoiser.from_vocoder, the absence of ATen compute and a weight-norm checkpoint
file."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import denoiser_reference as dr
import istftnet_reference as ir
from isp_tts_amd import graph, runtime, synth
from isp_tts_amd.istftnet import IstftNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_REL = 1e-4
BF16_FACTOR = 3.0
TF = runtime.ISTFTNET_TILE_FRAMES
DTYPES = (torch.float32, torch.bfloat16)
U = 2.0 ** -24

# name -> (B, T, lengths or None, strided): tests/test_gpu_hifigan.py's cases.  c8c8i stays at or below 64 frames in total.
CASES = {"b1_t1": (1, 1, None, False), "b1_t2": (1, 2, None, False), "ragged": (3, 43, [1, 7, 43], False),
         "zero_len": (4, 17, [5, 0, 17, 9], False), "strided": (2, 12, [12, 9], True), "no_len": (2, 5, None, False)}
DIMS = ("c8c8i", "odd", "n20")


# ------------------------------------------------------------------------------------------------ the head kernel alone
def _ola(per_frame: np.ndarray, n_fft: int, hop: int, power: int) -> np.ndarray:
    """sum_f w[t_f]^power per_frame[f] over the frames that cover each sample, trimmed as istft(center=True) trims."""
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    Fr = per_frame.shape[0]
    out = np.zeros(n_fft + hop * (Fr - 1))
    for f in range(Fr):
        out[f * hop:f * hop + n_fft] += win ** power * per_frame[f]
    return out[n_fft // 2:n_fft // 2 + hop * (Fr - 1)]


def _head_bound(x, w, bias, n_fft, hop, ps, y):
    """See test_head_kernel.  x float64 [1, C, n], y = conv_post's float64 output [1, n_fft + 2, F] -> bound float64 [hop n]."""
    C, H = x.shape[1], n_fft // 2
    p = F.pad(F.leaky_relu(x, 0.01), (1, 0), mode="reflect")
    e = (7 * C + 3) * U * (F.conv1d(p.abs(), w.abs(), padding=3)[0] + bias.abs()[:, None])          # [n_fft + 2, F]
    c = torch.full((H + 1, 1), 2.0, dtype=torch.float64)
    c[0], c[H] = 1.0, 1.0
    K = (n_fft + 22 + 4 * abs(ps)) * U
    per_frame = (c * torch.exp(y[0, :H + 1]) * (e[:H + 1] + abs(ps) * e[H + 1:] + K)).sum(0).numpy()  # [F]
    return _ola(per_frame, n_fft, hop, 1) / (n_fft * _ola(np.ones_like(per_frame), n_fft, hop, 2))


@pytest.mark.parametrize("n_fft, hop, ps", [(16, 4, 1.0), (8, 2, 1.0), (20, 5, math.pi)])
@pytest.mark.parametrize("C", [32, 64, 256])
def test_head_kernel(C, n_fft, hop, ps):
    """leaky-ReLU 0.01 -> reflection pad -> 7-tap C -> n_fft + 2 convolution -> exp / sin -> inverse STFT against float64.
    Bound per sample, a priori, in units of u = 2^-24:
      y      an fp32 fma chain of 7 C terms (here two of 7 C / 2 and their sum) plus the bias, on leaky-ReLU values that carry one
             rounding of their own, is within e = (7 C + 3) u (sum |x w| + |b|) of the exact y (Higham, gamma_n);
      mag    exp turns e into a RELATIVE error: |d mag| <= mag (e_k + 4 u) (expf: 2 ulp, first order in e);
      phase  sin is a contraction, then the scale: |d phase| <= |ps| (e'_k + 3 u);
      bin    |d Re|, |d Im| <= |d mag| + mag |d phase| + 4 u mag (cosf / sinf 2 ulp, the product);
      frame  g[t] = (1 / N) sum_k c_k (Re_k cos - Im_k sin), c = 1, 2, .., 2, 1: n_fft + 2 real terms, table entries rounded
             once, an fma chain of N terms and the window factor add (N + 4) u sum_k c_k mag_k;
      sample sum_f w g_f / sum_f w^2 over <= 4 frames: 3 + 3 additions and the division, 7 u of sum_f w |g_f| / env.
    Together |d audio[s]| <= sum_f w[t_f] E_f / (N env[s]),  E_f = sum_k c_k mag_k (e_k + |ps| e'_k + (N + 22 + 4 |ps|) u).
    An indexing error moves a sample by the size of the signal: the bound is asserted below 3 % of the batch's peak and below
    5 % of each utterance's own."""
    assert runtime.lib().ispk_istftnet_tile_frames() == TF
    g = torch.Generator().manual_seed(1000 * C + n_fft)
    H, NO = n_fft // 2, n_fft + 2
    w = ((torch.rand((NO, C, 7), generator=g) * 2 - 1) * 1.5 / (7 * C) ** 0.5).float()
    bias = torch.cat([torch.linspace(-2.0, 1.0, H + 1), torch.linspace(-2.0, 2.0, H + 1)]).float()
    w_img = w.permute(2, 0, 1).contiguous().to(DEV)
    table = runtime.istftnet_table(n_fft).to(DEV)
    worst = 0.0
    # (valid rows per utterance, len_mul, lengths given)
    for rows, len_mul, use_len in (([2, TF - 1, TF + 1], 1, True), ([TF - 2, TF, 2 * TF + 1], 1, True),
                                   ([2, TF, 2 * TF + 2], 2, True), ([TF + 1] * 3, 1, False)):
        T = max(rows) + (3 if use_len else 0)
        S = hop * T + 37
        x = (torch.rand((3, T, C), generator=g) * 2 - 1).float()
        xin = x.clone()
        want = torch.zeros((3, S), dtype=torch.float64)
        bound = torch.zeros((3, S), dtype=torch.float64)
        for b, n in enumerate(rows):
            xb = x[b, :n].double().T[None]
            a, y = ir.post(xb, w.double(), bias.double(), n_fft, hop, ps, want_y=True)
            assert a.shape == (1, hop * n)
            want[b, :hop * n] = a[0]
            bound[b, :hop * n] = torch.from_numpy(_head_bound(xb, w.double(), bias.double(), n_fft, hop, ps, y))
            xin[b, n:] = float("nan")                                    # padding: read through a select
        audio = torch.full((3, S), 7.0, device=DEV)
        alen = torch.full((3,), -1, dtype=torch.int64, device=DEV)
        ln = torch.tensor([n // len_mul for n in rows], dtype=torch.int64, device=DEV) if use_len else None
        runtime.istftnet_head(xin.reshape(3 * T, C).to(DEV), T, w_img, bias.to(DEV), table, n_fft, hop, audio, alen, lengths=ln,
                              len_mul=len_mul, slope=0.01, phase_scale=ps)
        assert alen.tolist() == [hop * n for n in rows]
        got = audio.cpu()
        err = (got.double() - want).abs()
        peak = float(want.abs().max())
        what = f"C={C} {n_fft}/{hop} rows={rows} len_mul={len_mul} len={use_len}"
        print(f"head {what}: max |err| {float(err.max()):.2e}, max bound {float(bound.max()):.2e}, peak {peak:.2f}, "
              f"worst err / bound {float((err / bound.clamp_min(1e-30)).max()):.1e}")
        assert peak > 0.2 and float(bound.max()) < 0.03 * peak, what
        assert not torch.isnan(got).any() and (err <= bound).all(), what
        worst = max(worst, float((err / bound.clamp_min(1e-30)).max()))
        for b, n in enumerate(rows):
            assert (got[b, hop * n:] == 0).all(), what
            assert float(bound[b].max()) < 0.05 * float(want[b].abs().max()), what
    print(f"head C={C} {n_fft}/{hop}: worst err / bound {worst:.1e}")


def test_head_short_and_bad_lengths():
    """One valid row has no reflection (torch raises): it counts as 0, as a length outside [0, T] does."""
    C, T, n_fft, hop = 32, 6, 16, 4
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, T, C), generator=g)
    w = (torch.randn((n_fft + 2, C, 7), generator=g) * 0.05).float()
    bias = torch.zeros(n_fft + 2)
    audio = torch.full((4, hop * T), 7.0, device=DEV)
    alen = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    ln = torch.tensor([1, -3, T + 1, 4], dtype=torch.int64, device=DEV)
    runtime.istftnet_head(x.reshape(4 * T, C).to(DEV), T, w.permute(2, 0, 1).contiguous().to(DEV), bias.to(DEV),
                          runtime.istftnet_table(n_fft).to(DEV), n_fft, hop, audio, alen, lengths=ln)
    assert alen.tolist() == [0, 0, 0, 16] and (audio[:3] == 0).all() and (audio[3, 16:] == 0).all()
    want = ir.post(x[3, :4].double().T[None], w.double(), bias.double(), n_fft, hop)[0]
    assert float((audio[3, :16].cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("n_fft, hop", [(16, 4), (8, 2), (20, 5)])
def test_reflection_pad_and_envelope_exact(n_fft, hop):
    """Weights zero but the centre tap of (log-magnitude of DC) <- channel 0, biases 0 on that channel and on the phases,
    -200 on the other log-magnitudes; channel 0 of a row is 0 ("on") or -20000 ("off": leaky-ReLU gives -200).  Frame f then
    has magnitude exp(0) = 1 on the DC bin with phase 0, or exp(-200) = 0 (exactly, in fp32), so
        audio[s] = sum_{f on} w[t_f] / N  /  sum_f w[t_f]^2
    over the frames of THE UTTERANCE that cover s, frame 0 being row 1 and frame i row i - 1.  A pad that is off by one frame
    moves the on / off pattern; an envelope taken from the batch's length changes the last n_fft / 2 samples of the shorter
    utterances.  The kernel's arithmetic on this input: w / N and w^2 each rounded once (the table), <= 3 additions each, one
    division; compared with float64 to 2 ulp in the first and last n_fft / 2 samples of every utterance (everywhere else as
    well: the interior has no more terms)."""
    C, H = 32, n_fft // 2
    rows = [2, 5, TF - 1, TF + 2]
    T = TF + 5
    g = torch.Generator().manual_seed(n_fft)
    x = (torch.rand((4, T, C), generator=g) * 2 - 1).float()
    on = torch.rand((4, T), generator=g) < 0.6
    for b, n in enumerate(rows):
        on[b, 0], on[b, 1] = True, False                     # frame 0 = row 1 is off, frame 1 = row 0 is on
        on[b, n - 1] = n != 2                                # the last frame
        if n > 3:
            on[b, n - 2] = False
    x[:, :, 0] = torch.where(on, 0.0, -20000.0)
    w = torch.zeros((n_fft + 2, C, 7))
    w[0, 0, 3] = 1.0
    bias = torch.zeros(n_fft + 2)
    bias[1:H + 1] = -200.0
    xin = x.clone()
    for b, n in enumerate(rows):
        xin[b, n:] = float("nan")
    audio = torch.full((4, hop * T), 7.0, device=DEV)
    ln = torch.tensor(rows, dtype=torch.int64, device=DEV)
    runtime.istftnet_head(xin.reshape(4 * T, C).to(DEV), T, w.permute(2, 0, 1).contiguous().to(DEV), bias.to(DEV),
                          runtime.istftnet_table(n_fft).to(DEV), n_fft, hop, audio, None, lengths=ln)
    got = audio.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(rows):
        frames_on = np.concatenate([on[b, 1:2].numpy(), on[b, :n].numpy()]).astype(np.float64)      # the reflection
        want = _ola(frames_on, n_fft, hop, 1) / (n_fft * _ola(np.ones(n + 1), n_fft, hop, 2))
        ref = ir.post(x[b, :n].double().T[None], w.double(), bias.double(), n_fft, hop)[0].numpy()
        assert np.abs(ref - want).max() <= 1e-12                                 # the closed form is the reference's value
        assert want[:H].max() > 0.2 / n_fft and want[-H:].max() > 0.2 / n_fft, "the edges must carry signal"
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got[b, :hop * n].astype(np.float64) - want) / ulp
        worst = max(worst, float(err.max()))
        assert err[:H].max() <= 2.0 and err[-H:].max() <= 2.0, f"{n_fft}/{hop} utterance {b}: edges {err[:H]} {err[-H:]} ulp"
        assert err.max() <= 2.0, f"{n_fft}/{hop} utterance {b}: {err.max()} ulp"
        assert (got[b, hop * n:] == 0).all()
    print(f"exact {n_fft}/{hop}: worst {worst:.2f} ulp")


# --------------------------------------------------------------------------------------------------------- whole model
def _mel(dims: str, case: str) -> tuple[torch.Tensor, torch.Tensor]:
    B, T, lens, strided = CASES[case]
    mel = synth.make_vocoder_mel(B, synth.ISTFTNET_DIMS[dims]["n_mels"], T, seed=len(case))
    if strided:    # [B, C, T] view of [B, T, C] storage
        mel = mel.transpose(1, 2).contiguous().transpose(1, 2)
    return mel, torch.tensor(lens if lens is not None else [T] * B, dtype=torch.int64)


@pytest.fixture(scope="module")
def models():
    out = {}
    for d in DIMS:
        cfg = synth.ISTFTNET_DIMS[d]
        sd = synth.make_istftnet_state_dict(cfg)
        out[d] = (sd, ir.build(sd, cfg), IstftNet.from_state_dict(sd, cfg).to(DEV).eval())
    return out


@pytest.fixture(scope="module")
def refs(models):
    """(dims, case) -> (ref64, ref_bf16): computed once, shared by the fp32 and bf16 tests."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cache = {}

    def get(d, case):
        if (d, case) not in cache:
            mel, ml = _mel(d, case)
            m = models[d][1]
            cache[(d, case)] = (ir.run_batch(m, mel, ml), ir.run_batch(m, mel, ml, ir.forward_bf16_operands))
        return cache[(d, case)]
    return get


def _run(voc: IstftNet, mel, ml, dtype=torch.float32, lengths=True):
    voc.set_compute_dtype(dtype)
    try:
        audio, alen = voc(mel.to(DEV), ml.to(DEV) if lengths else None)
        torch.cuda.synchronize()
    finally:
        voc.set_compute_dtype(torch.float32)
    return audio.cpu(), alen.cpu()


def _check_padding(audio, alen, ml, hop):
    assert torch.equal(alen, ml * hop)
    for b in range(audio.shape[0]):
        assert (audio[b, int(alen[b]):] == 0).all(), f"utterance {b}: non-zero samples past audio_len"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dims", DIMS)
def test_fp32_against_float64(models, refs, dims, case):
    mel, ml = _mel(dims, case)
    ref64, _ = refs(dims, case)
    voc = models[dims][2]
    hop = voc.hop_length
    audio, alen = _run(voc, mel, ml, lengths=CASES[case][2] is not None)
    assert audio.shape == (mel.shape[0], hop * mel.shape[2])
    _check_padding(audio, alen, ml, hop)
    worst = 0.0
    for b in range(mel.shape[0]):
        n = hop * int(ml[b])
        if n == 0:
            continue
        peak = float(ref64[b, :n].abs().max())
        assert 0.1 < peak < 4.0                        # informative: tests/test_istftnet_host.py has the full check
        err = float((audio[b, :n].double() - ref64[b, :n]).abs().max())
        worst = max(worst, err / peak)
        assert err <= FP32_REL * peak, f"{dims}/{case} utterance {b}: max err {err:.3e} > 1e-4 x peak {peak:.3e}"
    print(f"{dims}/{case}: fp32 worst max|err| / peak = {worst:.2e}")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dims", DIMS)
def test_bf16_against_float64_with_bf16_operands(models, refs, dims, case):
    mel, ml = _mel(dims, case)
    ref64, ref_bf = refs(dims, case)
    voc = models[dims][2]
    hop = voc.hop_length
    audio, alen = _run(voc, mel, ml, torch.bfloat16, lengths=CASES[case][2] is not None)
    _check_padding(audio, alen, ml, hop)
    worst = 0.0
    for b in range(mel.shape[0]):
        n = hop * int(ml[b])
        if n == 0:
            continue
        rounding = float((ref_bf[b, :n] - ref64[b, :n]).abs().max())
        err = float((audio[b, :n].double() - ref64[b, :n]).abs().max())
        worst = max(worst, err / rounding)
        assert err <= BF16_FACTOR * rounding, f"{dims}/{case} utterance {b}: bf16 err {err:.3e} > {BF16_FACTOR} x {rounding:.3e}"
    print(f"{dims}/{case}: bf16 worst err / bf16-operand error = {worst:.2f}")


# ------------------------------------------------------------------------------------------------------------ padding
@pytest.mark.parametrize("dims", DIMS)
def test_padding_semantics(models, dims):
    voc = models[dims][2]
    hop = voc.hop_length
    mel, ml = _mel(dims, "ragged")
    ml_d = ml.to(DEV)
    base, alen = voc(mel.to(DEV), ml_d)
    _check_padding(base.cpu(), alen.cpu(), ml, hop)
    zeroed = mel.clone()
    for fill in (0.0, float("nan"), 1e30):             # whatever lies past mel_len: bit-identical audio
        for b in range(3):
            zeroed[b, :, int(ml[b]):] = fill
        a, _ = voc(zeroed.to(DEV), ml_d)
        assert torch.equal(a, base), f"fill {fill}"
    # a ragged batch equals the same utterances run one by one, bit for bit
    for dtype in DTYPES:
        voc.set_compute_dtype(dtype)
        try:
            batch, _ = voc(mel.to(DEV), ml_d)
            for b in range(3):
                n = int(ml[b])
                alone, _ = voc(mel[b:b + 1, :, :n].to(DEV))
                assert torch.equal(alone[0], batch[b, :hop * n]), f"{dtype} utterance {b}"
        finally:
            voc.set_compute_dtype(torch.float32)
    # device lengths outside [0, T] give a zero row and audio_len 0
    T = mel.shape[2]
    bad = torch.tensor([-1, int(ml[1]), T + 1], dtype=torch.int64, device=DEV)
    a_bad, l_bad = voc(mel.to(DEV), bad)
    torch.cuda.synchronize()
    assert l_bad.tolist() == [0, hop * int(ml[1]), 0]
    assert (a_bad[0] == 0).all() and (a_bad[2] == 0).all() and torch.equal(a_bad[1], base[1])


def test_empty_batches_and_fp16_mel(models):
    voc = models["odd"][2]
    a, l = voc(torch.zeros((0, 20, 5), device=DEV))
    assert a.shape == (0, 60) and l.shape == (0,)
    a, l = voc(torch.zeros((2, 20, 0), device=DEV))
    assert a.shape == (2, 0) and l.tolist() == [0, 0]
    mel, _ = _mel("odd", "no_len")
    half, _ = voc(mel.half().to(DEV))
    up, _ = voc(mel.half().float().to(DEV))
    assert torch.equal(half, up) and float(half.abs().max()) > 0.1
    assert torch.equal(voc.infer(mel.to(DEV)), voc(mel.to(DEV))[0])


# ------------------------------------------------------------------------------------------- determinism and capture
@pytest.mark.parametrize("dims", ["odd", "n20"])
def test_determinism_and_graph_replay(models, dims):
    voc = models[dims][2]
    mel, ml = _mel(dims, "ragged")
    mel2, _ = _mel(dims, "ragged")
    mel2 = mel2.flip(2) * 0.9
    mel, ml, mel2 = mel.to(DEV), ml.to(DEV), mel2.to(DEV)
    for dtype in DTYPES:
        voc.set_compute_dtype(dtype)
        try:
            a1, _ = voc(mel, ml)
            a2, _ = voc(mel, ml)
            assert torch.equal(a1, a2)
            want2 = voc(mel2, ml)[0].clone()
            inp = mel.clone()
            out = voc.empty_outputs(mel.shape[0], mel.shape[2], DEV)
            g = graph.GraphedCall(lambda: voc(inp, ml, out=out))
            out[0].zero_()
            audio, _ = g.replay()
            torch.cuda.synchronize()
            assert torch.equal(audio, a1)
            inp.copy_(mel2)                          # new inputs through the captured call
            audio, _ = g.replay()
            torch.cuda.synchronize()
            assert torch.equal(audio, want2) and not torch.equal(want2, a1)
        finally:
            voc.set_compute_dtype(torch.float32)


def _acoustic_model():
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    return model.to(DEV).requires_grad_(False)


def test_text_to_pcm16_as_one_graph(models):
    """text -> mel -> iSTFTNet C8C8I -> conditioned -> PCM16, captured as one HIP graph: the replay equals the eager chain."""
    from isp_tts_amd.data import AudioConditioner, to_pcm16
    model, voc = _acoustic_model(), models["c8c8i"][2]
    cond = AudioConditioner(22050)
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 30), 2, dtype=torch.int64, device=DEV)
    wav = voc.empty_outputs(3, 64, DEV)
    assert wav[0].shape == (3, 64 * 256)
    out = cond.empty_outputs(3, wav[0].shape[1], DEV)
    pcm = torch.empty(wav[0].shape, dtype=torch.int16, device=DEV)

    def chain():
        mel, ao = model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=64)
        audio, audio_len = voc(mel, ao.dec_lengths, out=wav)
        r = cond(audio, audio_len, out=out)
        return to_pcm16(r["audio"], r["audio_len"], out=pcm), r

    chain()
    torch.cuda.synchronize()
    eager_pcm, eager = pcm.clone(), {k: v.clone() for k, v in out.items()}
    g = graph.GraphedCall(chain)
    pcm.zero_()
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pcm, eager_pcm)
    for k in eager:
        assert eager[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k
    assert (out["audio_len"] > 0).all() and pcm.abs().max() > 100


def test_score_infer_with_istftnet(models):
    from isp_tts_amd.acoustic.evaluator import SynthesisEvaluator
    from isp_tts_amd.data import AcousticFeatures
    model, voc = _acoustic_model(), models["c8c8i"][2]
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    pitch_hz = synth.make_stats_case("voices")["pitch"][:3, :64] * (torch.arange(64)[None] < inp["mel_len"][:, None])
    inputs = {"text": inp["text"].to(DEV), "text_len": inp["text_len"].to(DEV), "mel": inp["mel"].to(DEV),
              "mel_len": inp["mel_len"].to(DEV), "pitch_hz": pitch_hz.to(DEV)}
    kw = {"duration_target": torch.full((3, 30), 2, dtype=torch.int64, device=DEV), "steps": 4,
          "flow_noise": inp["flow_x0"].to(DEV), "max_dec_len": 64}
    ev, feats = SynthesisEvaluator(), AcousticFeatures(pitch_mean=0.0, pitch_std=1.0)
    got = ev.score_infer(model, inputs, vocoder=voc, features=feats, **kw)
    mel, ao = model.infer(inputs["text"], text_lengths=inputs["text_len"], **kw)
    audio, alen = voc(mel, ao.dec_lengths)
    assert torch.equal(alen, ao.dec_lengths * voc.hop_length)
    pitch = feats(audio, alen)["pitch"]
    want = ev(mel, ao.dec_lengths, inputs["mel"], inputs["mel_len"], pitch, inputs["pitch_hz"])
    torch.cuda.synchronize()
    assert list(got) == list(want) and len(got) == 4
    assert all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in got)
    for k in ("metrics/mcd_dtw_13", "metrics/vuv_error", "metrics/length_ratio"):
        assert bool(torch.isfinite(got[k])), got
    # f0_rmse_cents is NaN by definition when no aligned pair of frames is voiced on both sides (tests/dtw_reference.py), which
    # a generator with random weights may give; it is never infinite
    assert not bool(torch.isinf(got["metrics/f0_rmse_cents"])), got


def test_denoiser_from_vocoder(models):
    from isp_tts_amd.denoiser import Denoiser
    voc = models["odd"][2]
    hop = voc.hop_length
    frames = max(88, -(-2048 // hop))
    den = Denoiser.from_vocoder(voc, mode="zeros", strength=0.25)
    assert den.bias_spec.is_cuda and den.bias_spec.shape == (1, 513, 1) and den.strength == 0.25
    audio, alen = voc(torch.zeros((1, voc.n_mels, frames), device=DEV))
    n = int(alen[0])
    assert n == frames * hop >= 2048
    want = np.abs(dr.stft(audio[0, :n].cpu().double().numpy())[0])          # frame 0 of the vocoder's own output, float64
    got = den.bias_spec.flatten().cpu().double().numpy()
    assert float(want.max()) > 0
    assert (np.abs(got - want) <= 2.0 ** -24 * want * (1 + 1e-9) + 1e-30).all()
    out, out_len = den(audio, alen)
    torch.cuda.synchronize()
    assert out.shape == audio.shape and torch.equal(out_len, alen) and bool(torch.isfinite(out).all())


def test_istftnet_issues_no_aten_compute_ops(models):
    from torch.utils._python_dispatch import TorchDispatchMode
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream")
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not str(func).startswith(harmless):
                seen.append(str(func))
            return func(*args, **(kwargs or {}))

    for dims in ("odd", "n20"):
        voc = models[dims][2]
        mel, ml = _mel(dims, "ragged")
        ml = ml.to(DEV)
        for m in (mel.to(DEV), mel.to(DEV).half()):
            for dtype in DTYPES:
                voc.set_compute_dtype(dtype)
                try:
                    voc(m, ml)                      # stages the weight images outside the watched call
                    torch.cuda.synchronize()
                    with Watch():
                        voc(m, ml)
                        voc.infer(m)
                    torch.cuda.synchronize()
                finally:
                    voc.set_compute_dtype(torch.float32)
                assert not seen, f"{dims} {m.dtype} / {dtype}: PyTorch compute ops inside IstftNet: {sorted(set(seen))}"


def test_weight_norm_checkpoint_through_from_pretrained(models, tmp_path):
    """A {"generator": ...} file with weight_g / weight_v gives the audio of the model built from the folded plain weights."""
    cfg = synth.ISTFTNET_DIMS["n20"]
    sd = synth.make_istftnet_state_dict(cfg, weight_norm="g_v")
    torch.save({"generator": sd}, tmp_path / "g_00975000")
    loaded = IstftNet.from_pretrained(tmp_path / "g_00975000", cfg).to(DEV).eval()
    assert loaded.phase_scale == math.pi and loaded.n_fft == 20
    folded = {k: v.float() for k, v in ir.fold(sd).items()}
    plain = IstftNet(**cfg)
    plain.load_state_dict(folded, strict=True)
    plain = plain.to(DEV).eval()
    mel, ml = _mel("n20", "ragged")
    a1, l1 = loaded(mel.to(DEV), ml.to(DEV))
    a2, l2 = plain(mel.to(DEV), ml.to(DEV))
    assert torch.equal(a1, a2) and torch.equal(l1, l2)
    ref = models["n20"][2](mel.to(DEV), ml.to(DEV))[0]          # and it is the plain-weight model to rounding
    assert float((a1 - ref).abs().max()) <= FP32_REL * float(ref.abs().max())
