"""GPU: the BigVGAN generator (isp_tts_amd.bigvgan.BigVGan: csrc/bigvgan.hip + the HiFi-GAN convolution kernels with slope 1 +
ispk_vocoder_unfold + the GEMM entry).

Kernel level.  ispk_snake_aa_f32 alone against the float64 padded conv_transpose1d / conv1d form of tests/bigvgan_reference.py:
  * indexing, exact: al = 0 and inv_b = 1 make the snake term exactly 0, the taps are small integers (non-symmetric, different
    for the two filters) and x integers with |x| <= 8, so every product and sum is exact in fp32: torch.equal, at the lengths
    1, 2, 3, 5, 6, TM - 1, TM, TM + 1, 2 TM + 1 (TM = runtime.SNAKE_AA_TILE_ROWS, the rows of a workgroup) and around the 16
    rows of a thread's tile, with len_mul 1 and 2 and without lengths, padded row strides, NaN past the lengths;
  * non-linear: a per-element a-priori bound (test_snake_aa_against_float64) whose only free constant, K_SIN, was measured
    once on gfx950: K_SIN_MEASURED below.
ispk_hifigan_post_clamp_f32 against float64 with test_gpu_hifigan.test_post_kernel's bound less its tanh term.

Whole model against the float64 module run utterance by utterance.  Bounds, per utterance, over its samples m < hop mel_len
(DESIGN.md 4.13, 4.19, 4.20):
  fp32   max |audio - ref64| <= 1e-4 x max |ref64|
  bf16   max |audio - ref64| <= BF16_FACTOR x max |ref_bf16 - ref64|, ref_bf16 = the float64 module with the input and the
         weight of every convolution but conv_post rounded to bf16 (bigvgan_reference.forward_bf16_operands)
and exactly 0 at and past hop mel_len.  Measured on gfx950: fp32 worst err / peak 4.3e-6 (base), 1.9e-6 (odd), 1.6e-6 (odd2);
bf16 worst err / bf16-operand error 1.27 (base), 1.11 (odd), 1.02 (odd2).

Then the padding semantics, determinism, graph capture (alone, and behind AcousticModel.infer with the conditioner and the
PCM16 export), the absence of ATen compute and a weight-norm checkpoint file with its config.json."""
import json

import pytest
import torch
import torch.nn.functional as F

import bigvgan_reference as br
from isp_tts_amd import graph, runtime, synth
from isp_tts_amd.bigvgan import BigVGan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_REL = 1e-4
BF16_FACTOR = 3.0
TM = runtime.SNAKE_AA_TILE_ROWS
DTYPES = (torch.float32, torch.bfloat16)
EPS = 2.0 ** -24
# The smallest K_SIN for which the float64 reference bounds the kernel in test_snake_aa_against_float64, measured on gfx950
# (the test prints it): -2.65 (C = 32), -1.51 (C = 64), -0.27 (C = 256).  It is negative: the kernel's whole error lies inside
# the bound's other terms, which are worst cases of fma chains.  Asserted with 4 x the largest, at least 2: other gfx950
# machines and compiler versions.
K_SIN_MEASURED = -0.27
K_SIN = max(4.0 * K_SIN_MEASURED, 2.0)

# name -> (B, T, lengths or None, strided): test_gpu_hifigan.CASES.  "base" stays at or below 64 frames in total.
CASES = {"b1_t1": (1, 1, None, False), "b1_t2": (1, 2, None, False), "ragged": (3, 43, [1, 7, 43], False),
         "zero_len": (4, 17, [5, 0, 17, 9], False), "strided": (2, 12, [12, 9], True), "no_len": (2, 5, None, False)}
DIMS = tuple(synth.BIGVGAN_DIMS)
# lengths of the activation kernel's tests, three utterances to a batch: the issue's list, then the edges of a thread's tile
LENGTHS = ([1, TM - 1, 2 * TM + 1], [2, TM, 5], [3, TM + 1, 6], [15, 16, 17], [31, 33, 48])


# ------------------------------------------------------------------------------------------- activation kernel, exact
def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _run_snake(x, lens, al, inv_b, taps, len_mul=1, use_len=True, pad_x=8, pad_o=4, sentinel=7.0):
    """x float64 [B, T, C] (NaN past the lengths) -> (out [B, T, C], the untouched padding columns [B*T, pad_o])."""
    B, T, C = x.shape
    xs = torch.full((B * T, C + pad_x), float("nan"))
    xs[:, :C] = x.float().reshape(B * T, C)
    os_ = torch.full((B * T, C + pad_o), sentinel, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV) if use_len else None
    got = runtime.snake_aa(xs.to(DEV)[:, :C], T, al.float().to(DEV), inv_b.float().to(DEV), taps.float().to(DEV),
                           out=os_[:, :C], lengths=ln, len_mul=len_mul)
    assert got.data_ptr() == os_.data_ptr()
    torch.cuda.synchronize()
    return os_[:, :C].cpu().reshape(B, T, C), os_[:, C:].cpu()


@pytest.mark.parametrize("C", [32, 64, 256])
def test_snake_aa_indexing_exact(C):
    assert runtime.lib().ispk_snake_aa_tile_rows() == TM
    fu = torch.tensor([1, -2, 0, 2, -1, 1, 2, -2, 1, 0, -1, 2], dtype=torch.float64)
    fd = torch.tensor([-1, 2, 1, -2, 2, 0, 1, -1, -2, 1, 2, -1], dtype=torch.float64)
    assert not torch.equal(fu, fu.flip(0)) and not torch.equal(fd, fd.flip(0)) and not torch.equal(fu, fd)
    al, inv_b = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    for lens in LENGTHS:
        for len_mul, use_len in ((1, True), (2, True), (1, False)):
            T = len_mul * max(lens) + 3
            valid = [len_mul * n if use_len else T for n in lens]
            x = _ints((3, T, C), -8, 8, 100 * C + 10 * lens[0] + len_mul)
            want = torch.zeros((3, T, C), dtype=torch.float64)
            xin = x.clone()
            for b in range(3):
                n = valid[b]
                want[b, :n] = br.snake_aa(x[b, :n].T[None], al, inv_b, fu, fd)[0].T
                xin[b, n:] = float("nan")                                     # padding: never read
            got, pad = _run_snake(xin, lens, al, inv_b, torch.cat([fu, fd]), len_mul, use_len)
            what = f"C={C} lens={lens} len_mul={len_mul} len={use_len}"
            assert float(want.abs().max()) > 100, what
            assert torch.equal(got.double(), want), f"{what}: max |diff| {float((got - want).abs().nan_to_num(1e9).max())}"
            assert (pad == 7.0).all(), f"{what}: columns past C were written"
            for b in range(3):
                assert (got[b, valid[b]:] == 0).all(), what              # the sentinel came back as zeros


def test_snake_aa_out_of_range_lengths_count_as_zero():
    C, T = 32, 40
    x = _ints((3, T, C), -8, 8, 1)
    fu, fd = _ints((12,), -2, 2, 2), _ints((12,), -2, 2, 3)
    al, inv_b = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    got, _ = _run_snake(x, [3, 6, -1], al, inv_b, torch.cat([fu, fd]), len_mul=8)   # 24 rows; 48 > T and -8 count as 0
    want = br.snake_aa(x[0, :24].T[None], al, inv_b, fu, fd)[0].T
    assert torch.equal(got[0, :24].double(), want) and (got[0, 24:] == 0).all() and (got[1:] == 0).all()


# ------------------------------------------------------------------------------- activation kernel, against float64
def _abs_aa(x_abs, fu_abs):
    """2 sum |fu| |x| per upsampled position: the padded form on magnitudes.  x_abs [1, C, n] -> [1, C, 2n]."""
    C = x_abs.shape[1]
    u = F.pad(x_abs, (5, 5), mode="replicate")
    return 2 * F.conv_transpose1d(u, fu_abs.reshape(1, 1, 12).expand(C, 1, 12), stride=2, groups=C)[..., 15:-15]


def _down_abs(a, fd_abs):
    C = a.shape[1]
    return F.conv1d(F.pad(a, (5, 6), mode="replicate"), fd_abs.reshape(1, 1, 12).expand(C, 1, 12), stride=2, groups=C)


@pytest.mark.parametrize("C", [32, 64, 256])
def test_snake_aa_against_float64(C):
    """x uniform in [-3, 3], al in [0.5, 4], inv_b in [0.25, 2] per channel, the kaiser-sinc taps (as fp32, in the kernel and in
    the reference).  Bound per element, a priori, in units of 2^-24 (fp32 round-off u):
      u[s]: a 6-term fma chain and an exact doubling: |du| <= 7 u sum |2 fu x|                                  (Higham, gamma_n)
      a[s] = u + inv_b sin(al u)^2: the product al u is rounded (u |al u|) and inherits al du; sin^2 is 1-Lipschitz in its
             argument; sinf, the square, the product with inv_b and their roundings are K_SIN u on a value <= 1:
             |da| <= du + inv_b (u |al u| + al du + K_SIN u)
      y[t]:  |dy| <= sum_j |fd_j| da[2t + j - 5] + 13 u sum_j |fd_j a|      (a 12-term chain, and the rounding of a itself)
    K_SIN is not derived: the smallest value for which this bound holds was measured once (K_SIN_MEASURED, printed below on
    every run) and the assertion uses K_SIN = max(4 K_SIN_MEASURED, 2) = 2.  Measured on gfx950: -2.65, -1.51 and -0.27 for
    C = 32, 64 and 256 (the bound holds without the term); the largest bound is 2.3e-5 against a peak of 5.0 - 5.3.
    The bound must stay below 1e-5 of the signal's peak, or it would say nothing: torch's own fp32 evaluation of this op is
    1.7e-7 of the peak from float64, an indexing error moves an element by the size of the signal."""
    g = torch.Generator().manual_seed(C)
    taps32 = br.kaiser_sinc_taps().float()
    fu = fd = taps32.double()
    al = (0.5 + 3.5 * torch.rand(C, generator=g)).float()
    inv_b = (0.25 + 1.75 * torch.rand(C, generator=g)).float()
    ald, ibd = al.double()[None, :, None], inv_b.double()[None, :, None]
    k_min, worst_bound, peak_all = -1e30, 0.0, 0.0
    failures = []
    for lens in LENGTHS:
        T = max(lens) + 3
        x = (torch.rand((3, T, C), generator=g) * 6 - 3).float().double()
        want = torch.zeros((3, T, C), dtype=torch.float64)
        base = torch.zeros((3, T, C), dtype=torch.float64)       # the bound without its K_SIN term
        coef = torch.ones((3, T, C), dtype=torch.float64)        # d bound / d K_SIN
        xin = x.clone()
        for b in range(3):
            n = lens[b]
            xb = x[b, :n].T[None]
            # u, a in float64 from the padded form
            up = F.pad(xb, (5, 5), mode="replicate")
            u = 2 * F.conv_transpose1d(up, fu.reshape(1, 1, 12).expand(C, 1, 12), stride=2, groups=C)[..., 15:-15]
            a = u + ibd * torch.sin(ald * u) ** 2
            du = 7 * EPS * _abs_aa(xb.abs(), fu.abs())
            da0 = du + ibd * (EPS * (ald * u).abs() + ald * du)
            want[b, :n] = br.snake_aa(xb, al.double(), inv_b.double(), fu, fd)[0].T
            base[b, :n] = (_down_abs(da0, fd.abs()) + 13 * EPS * _down_abs(a.abs(), fd.abs()))[0].T
            coef[b, :n] = (_down_abs((ibd * EPS).expand_as(u).contiguous(), fd.abs()))[0].T
            xin[b, n:] = float("nan")
        got, _ = _run_snake(xin, lens, al.double(), inv_b.double(), torch.cat([taps32, taps32]).double())
        err = (got.double() - want).abs()
        for b in range(3):
            n = lens[b]
            assert (got[b, n:] == 0).all(), f"C={C} lens={lens}"
            e, bs, cf = err[b, :n], base[b, :n], coef[b, :n]
            k_min = max(k_min, float(((e - bs) / cf).max()))
            bound = bs + K_SIN * cf
            worst_bound, peak_all = max(worst_bound, float(bound.max())), max(peak_all, float(want[b, :n].abs().max()))
            if not bool((e <= bound).all()):
                failures.append(f"lens={lens} b={b}: max err {float(e.max()):.3e}, worst err / bound {float((e / bound).max()):.2f}")
    print(f"snake_aa C={C}: smallest K_SIN that bounds the kernel = {k_min:.3f} (asserting with {K_SIN}); max bound "
          f"{worst_bound:.2e}, peak {peak_all:.2f}")
    assert worst_bound <= 1e-5 * peak_all, f"vacuous bound {worst_bound:.2e} against a peak of {peak_all:.2f}"
    assert not failures, failures


# ------------------------------------------------------------------------------------------- post kernel, clamp variant
@pytest.mark.parametrize("C", [32, 64, 256])
def test_post_clamp_kernel(C):
    """7-tap C -> 1 convolution -> clamp(., -1, 1) against float64, with and without a leaky-ReLU on load.  Bound per sample, a
    priori: an fp32 fma chain of n = 7 C terms plus the bias is within (n + 1) 2^-24 of sum |x_i w_i| + |bias| (Higham,
    gamma_n) and the clamp is a contraction that rounds nothing: test_gpu_hifigan.test_post_kernel's bound less its tanh term.
    The weights are scaled so that the clamp acts on both sides and leaves most samples alone; the bias takes out the offset
    that the leaky-ReLU's mean, (1 - slope) / 4 on uniform [-1, 1], gives the sum, so that both rails are reached."""
    g = torch.Generator().manual_seed(C)
    Tp = runtime.HIFIGAN_TILE_ROWS
    L, S_extra = 2 * Tp + 1, 37
    T, lens = L + 3, [1, L, L + 1]
    x = (torch.rand((3, T, C), generator=g) * 2 - 1).float()
    w = ((torch.rand((1, C, 7), generator=g) * 2 - 1) * 3.0 / (7 * C) ** 0.5).float()
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV)
    for slope in (1.0, 0.01):
        bias = torch.tensor([0.1 - (1 - slope) / 4 * float(w.double().sum())])
        xin = x.clone()
        want = torch.zeros((3, T + S_extra), dtype=torch.float64)
        bound = torch.zeros((3, T + S_extra), dtype=torch.float64)
        pre = []
        for b in range(3):
            a = F.leaky_relu(x[b, :lens[b]].double(), slope).T[None]
            v = F.conv1d(a, w.double(), bias.double(), padding=3)[0, 0]
            pre.append(v)
            want[b, :lens[b]] = v.clamp(-1.0, 1.0)
            bound[b, :lens[b]] = (7 * C + 1) * EPS * (F.conv1d(a.abs(), w.double().abs(), padding=3)[0, 0] + 0.1)
            xin[b, lens[b]:] = float("nan")
        pre = torch.cat(pre)
        hi, lo, mid = float((pre >= 1).double().mean()), float((pre <= -1).double().mean()), float((pre.abs() < 1).double().mean())
        assert hi >= 0.01 and lo >= 0.01 and mid >= 0.5, f"slope {slope}: clamped shares +{hi:.3f} -{lo:.3f}, untouched {mid:.3f}"
        xd, wd, bd = xin.reshape(3 * T, C).to(DEV), w[0].t().contiguous().to(DEV), bias.to(DEV)
        audio = torch.full((3, T + S_extra), 7.0, device=DEV)
        alen = torch.empty((3,), dtype=torch.int64, device=DEV)
        runtime.hifigan_post(xd, T, wd, bd, audio, alen, lengths=ln, slope=slope, final_clamp=True)
        assert alen.tolist() == lens
        got = audio.cpu()
        err = (got.double() - want).abs()
        print(f"post clamp C={C} slope={slope}: max |err| = {float(err.max()):.2e}, max bound {float(bound.max()):.2e}, "
              f"clamped +{hi:.3f} -{lo:.3f}")
        assert float(bound.max()) < 5e-3 and (err <= bound).all()
        assert float(got.max()) == 1.0 and float(got.min()) == -1.0
        for b in range(3):
            assert (got[b, lens[b]:] == 0).all()
        # the tanh entry on the same inputs: the option's default is the entry as it was, called directly
        t1 = torch.full((3, T + S_extra), 7.0, device=DEV)
        t2 = torch.full((3, T + S_extra), 7.0, device=DEV)
        runtime.hifigan_post(xd, T, wd, bd, t1, None, lengths=ln, slope=slope, final_clamp=False)
        rc = runtime.lib().ispk_hifigan_post_f32(xd.data_ptr(), xd.stride(0), wd.data_ptr(), bd.data_ptr(), ln.data_ptr(), 1,
                                                 t2.data_ptr(), t2.stride(0), None, 3, T, T + S_extra, C, slope,
                                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(t1, t2)
        tanh_want = torch.zeros_like(want)
        o = 0
        for b in range(3):
            tanh_want[b, :lens[b]] = torch.tanh(pre[o:o + lens[b]])
            o += lens[b]
        assert ((t1.cpu().double() - tanh_want).abs() <= bound + 2.0 ** -22).all()      # test_post_kernel's own bound


# --------------------------------------------------------------------------------------------------------- whole model
def _mel(dims: str, case: str) -> tuple[torch.Tensor, torch.Tensor]:
    B, T, lens, strided = CASES[case]
    mel = synth.make_vocoder_mel(B, synth.BIGVGAN_DIMS[dims]["n_mels"], T, seed=len(case))
    if strided:    # [B, C, T] view of [B, T, C] storage
        mel = mel.transpose(1, 2).contiguous().transpose(1, 2)
    return mel, torch.tensor(lens if lens is not None else [T] * B, dtype=torch.int64)


@pytest.fixture(scope="module")
def models():
    out = {}
    for d in DIMS:
        cfg = synth.BIGVGAN_DIMS[d]
        sd = synth.make_bigvgan_state_dict(cfg)
        out[d] = (sd, br.build(sd, cfg), BigVGan.from_state_dict(sd, cfg).to(DEV).eval())
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
            cache[(d, case)] = (br.run_batch(m, mel, ml), br.run_batch(m, mel, ml, br.forward_bf16_operands))
        return cache[(d, case)]
    return get


def _run(voc: BigVGan, mel, ml, dtype=torch.float32, lengths=True):
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


def _check_reference_is_informative(voc, ref64, ml, hop, what):
    """A tanh in its flat part or a near-silent output would hide errors; so would a clamp that holds most samples or none.
    Under the clamp the shares are taken over the case's samples together, where there are at least 100 of them (1 % of fewer
    is less than one sample): at least 1 % at each rail, at least half strictly inside."""
    if voc.use_tanh_at_final:
        for b in range(ref64.shape[0]):
            n = hop * int(ml[b])
            if n:
                peak, rms = float(ref64[b, :n].abs().max()), float(ref64[b, :n].pow(2).mean().sqrt())
                assert peak < 0.95 and rms > 0.02, f"{what} utterance {b}: reference peak {peak:.3f} rms {rms:.3f}"
        return
    v = torch.cat([ref64[b, :hop * int(ml[b])] for b in range(ref64.shape[0])])
    hi, lo, mid = float((v >= 1).double().mean()), float((v <= -1).double().mean()), float((v.abs() < 1).double().mean())
    assert mid >= 0.5, f"{what}: {mid:.3f} of the reference's samples inside the clamp"
    if v.numel() >= 100:
        assert hi >= 0.01 and lo >= 0.01, f"{what}: clamped shares +{hi:.3f} -{lo:.3f}"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dims", DIMS)
def test_fp32_against_float64(models, refs, dims, case):
    mel, ml = _mel(dims, case)
    ref64, _ = refs(dims, case)
    voc = models[dims][2]
    hop = voc.hop_length
    _check_reference_is_informative(voc, ref64, ml, hop, f"{dims}/{case}")
    audio, alen = _run(voc, mel, ml, lengths=CASES[case][2] is not None)
    assert audio.shape == (mel.shape[0], hop * mel.shape[2])
    _check_padding(audio, alen, ml, hop)
    worst = 0.0
    for b in range(mel.shape[0]):
        n = hop * int(ml[b])
        if n == 0:
            continue
        peak = float(ref64[b, :n].abs().max())
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
    assert a.shape == (0, 30) and l.shape == (0,)
    a, l = voc(torch.zeros((2, 20, 0), device=DEV))
    assert a.shape == (2, 0) and l.tolist() == [0, 0]
    mel, _ = _mel("odd", "no_len")
    half, _ = voc(mel.half().to(DEV))
    up, _ = voc(mel.half().float().to(DEV))
    assert torch.equal(half, up)
    assert torch.equal(voc.infer(mel.to(DEV)), voc(mel.to(DEV))[0])


# ------------------------------------------------------------------------------------------- determinism and capture
@pytest.mark.parametrize("dims", ["odd", "odd2"])
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
    """text -> mel -> BigVGAN base -> conditioned -> PCM16, captured as one HIP graph: the replay equals the eager chain."""
    from isp_tts_amd.data import AudioConditioner, to_pcm16
    model, voc = _acoustic_model(), models["base"][2]
    cond = AudioConditioner(22050)
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 30), 2, dtype=torch.int64, device=DEV)
    wav = voc.empty_outputs(3, 64, DEV)
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


def test_bigvgan_issues_no_aten_compute_ops(models):
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

    for dims in ("odd", "odd2"):
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
                assert not seen, f"{dims} {m.dtype} / {dtype}: PyTorch compute ops inside BigVGan: {sorted(set(seen))}"


def test_weight_norm_checkpoint_through_from_pretrained(models, tmp_path):
    """A {"generator": ...} file with weight_g / weight_v and the config.json beside it give the audio of the model built from
    the folded plain weights."""
    cfg = synth.BIGVGAN_DIMS["odd2"]
    sd = synth.make_bigvgan_state_dict(cfg, weight_norm="g_v")
    torch.save({"generator": sd}, tmp_path / "bigvgan_generator.pt")
    official = {k: (list(map(list, v)) if k == "resblock_dilation_sizes" else list(v) if isinstance(v, tuple) else v)
                for k, v in cfg.items() if k != "n_mels"}
    (tmp_path / "config.json").write_text(json.dumps(dict(official, num_mels=cfg["n_mels"], use_cuda_kernel=False)))
    loaded = BigVGan.from_pretrained(tmp_path / "bigvgan_generator.pt").to(DEV).eval()
    assert loaded.config() == cfg
    folded = {k: v.float() for k, v in br.fold(sd).items()}
    plain = BigVGan(**cfg)
    plain.load_state_dict(folded, strict=True)
    plain = plain.to(DEV).eval()
    mel, ml = _mel("odd2", "ragged")
    a1, l1 = loaded(mel.to(DEV), ml.to(DEV))
    a2, l2 = plain(mel.to(DEV), ml.to(DEV))
    assert torch.equal(a1, a2) and torch.equal(l1, l2)
    ref = models["odd2"][2](mel.to(DEV), ml.to(DEV))[0]        # and it is the plain-weight model to rounding
    assert float((a1 - ref).abs().max()) <= FP32_REL * float(ref.abs().max())
