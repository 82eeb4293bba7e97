"""The aligner front end, forward and backward (the aligner half of csrc/aligner.hip, all of csrc/aligner_bwd.hip), each entry point
against its float64 reference (tests/aligner_reference.py, proved against the oracle and float64 autograd by
tests/test_aligner_reference_host.py), through the `runtime` wrappers, at the smallest shapes that reach every branch.  Every test
runs its kernel twice on the same inputs (same bits) and checks that the inputs are unchanged.

Branches per entry point
  ispk_pad_rows_f32, output modes fp32 / bf16 / split fp16 planes                                               (B, T, C)
    pad_rows_kernel (channel-last input, one thread per output element, 256 per workgroup)
      (1, 1, 1)     5 outputs                              (2, 28, 4)   256 outputs: exactly one workgroup
      (2, 28, 5)    320 outputs: a second, partial one     (3, 37, 80)  x the column slice [:, :, 8:88] of a [3, 37, 96] tensor
    pad_rows_cf_kernel (channel-first input with stride_t == 1 < stride_c; 32 x 32 tiles over (T + 4, C)): x is the time slice
    [:, :, :T] of a [B, C, T + 3] tensor, so stride_c > 1 at T = 1 too (a contiguous [B, C, 1] goes to the kernel above)
      (2, 28, 32)   one full tile                          (2, 29, 33)  one more row and column of tiles, each of width 1
      (3, 27, 31)   one short in both directions           (1, 1, 80)   T + 4 = 5 rows; three channel tiles, the last of 16
    (65536, 1, 2) channel-first: B > 65535 sends it to pad_rows_kernel, 4 floats between neighbouring threads; 655,360 outputs
    lengths 0, 1, T and T + 3 (clamped to T) under both kernels; 1e6 (the split mode clamps it), +-65504 and 1e-7 among the values
  ispk_masked_instnorm_f32, the same three output modes (16 time lanes x 64 channels; the eight-fold trip of the mean pass, the
  variance pass - the write loop runs over all T + 4 rows - goes while a lane's frame + 112 < n)                 (B, T, C) lengths
    (2, 1, 80)     (1, 0)          n = 1 = T (0 is clamped to 1): variance exactly 0, the output is exactly bias
    (3, 15, 1)     (15, 1, 20)     n = 15 = T: lane 15 idle; n = 1 < T; 20 clamped; one channel: 63 idle channel lanes
    (3, 16, 64)    (16, 15, 1)     n = 16 = T: one frame per lane; 15 < T; one full channel block
    (3, 17, 65)    (17, 1, 9)      n = 17 = T: lane 0 takes two tail frames; a second channel block of one channel
    (3, 112, 63)   (112, 16, 17)   n = 112 = T: tail loop only, 7 frames per lane; 16 and 17 < T
    (2, 113, 160)  (113, 112)      n = 113 = T: lane 0 alone takes the trip (and nothing after it); 112 < T; three channel blocks
    (3, 129, 64)   (129, 113, 0)   n = 129 = T: every lane takes the trip, the tail is frame 128 alone; 113 < T
    (3, 300, 80)   (300, 129, 17)  n = 300 = T: two trips, then 2 or 3 tail frames; 129 < T
    (2, 301, 1)    (300, 15)       n = 300 < T
    rows t >= n of the input (the four scratch rows included) hold NaN; with C >= 3 channel 1 is constant over its valid frames
    and channel 2 is 1000 +- 2^-6 (2^-5 at n = 300) with mean exactly 1000: see aligner_reference's docstring for why not 1e-2
  ispk_masked_instnorm_bwd_f32 (plain loops over t < n; instnorm_param_sum_kernel adds the utterances' partials in order)
    (1, 17, 65)  B = 1; two channel blocks      (3, 33, 64)  lengths (33, 16, 1)      (3, 16, 80)  lengths (15, 0, 20), clamped
    (1, 300, 1)  19 frames per lane             (2, 9, 260)  five channel blocks; a second workgroup of the parameter sum (4 live)
    y and d_out hold NaN in the rows t >= n, the workspace is NaN-filled; a short workspace is refused with -2, NULL with -1
  ispk_aligner_scores_f32 / _fast_f32 (aligner_scores_kernel<NB, false | true>, NB = ceil(L / 32); a wave owns 32 mel rows, a
  workgroup 64)                                                                              (B, M, L) text_len mel_len
    (2, 31, 1)     (1, 0) (31, 0)             NB 1: one key, the LDS is the two transpose patches; lengths 0, clamped to 1
    (2, 1, 31)     (31, 17) (1, 1)            NB 1, scalar stores; M = 1
    (3, 32, 32)    (32, 37, 1) (32, 39, 20)   NB 1, vector stores; wave 1 has no live row; lengths above the size, clamped
    (2, 33, 33)    (33, 32) (33, 7)           NB 2, block 1 has one live key; wave 1 has one live row; q_stride_b = 2 (M + 4) 128
    (2, 64, 64)    (64, 40) (71, 33)          NB 2 full; M + 7 clamped; q scaled so that |scale q.k| reaches 80
    (2, 65, 65)    (65, 0) (65, 64)           NB 3; a second workgroup with one live row
    (2, 130, 100)  (100, 57) (130, 77)        NB 4, the bench's L; three workgroups, the last with two live rows
    (2, 33, 129)   (129, 100) (33, 0)         NB 5
    (2, 65, 160)   (165, 130) (65, 40)        NB 5, the largest L at which two workgroups share a CU; L + 5 clamped
    (2, 31, 161)   (161, 33) (31, 1)          NB 6
    (2, 32, 193)   (193, 150) (32, 9)         NB 7
    (2, 64, 226)   (226, 101) (64, 50)        NB 8, L % 4 == 2: scalar stores with a two-element last group
    (2, 1, 257)    (257, 200) (1, 1)          NB 9
    (2, 130, 289)  (289, 270) (130, 100)      NB 10
    (3, 65, 320)   (320, 325, 1) (65, 0, 72)  NB 10, the documented maximum: 160 KiB of dynamic LDS
    the four scratch rows of q and k hold NaN; L = 321 is refused with -2, D = 64 with -4, q offset by 4 bytes with -3
  ispk_aligner_scores_bwd_f32 (one wave per (b, m) row, four rows per workgroup, columns strided by 64)        (B, M, L)
    (1, 1, 1)    B M = 1; one column: the reference is 0      (2, 2, 64)   B M = 4: one full workgroup; lengths 0 and M + 3
    (1, 4, 63)   L4 > L; text_len above L; row 3 past mel_len   (1, 5, 65)   a second workgroup with one live wave; L4 > L, M4 > M
    (5, 1, 130)  five utterances of one row; three trips        (1, 5, 320)  five trips        (3, 33, 65)  rows past mel_len
    each with d_soft alone, d_logits alone and both (both NULL: -1); logits and soft are the float64 forward rounded to fp32
  ispk_soft_average_bwd_f32 (soft_average_cols_kernel: one wave per (b, l) column, four per workgroup, frames strided by 64;
  soft_average_bwd_kernel: one thread per element, 256 per workgroup)                                          (B, M, L)
    (1, 1, 4)    M = 1: lane 0 alone has a frame     (1, 63, 4)   B L = 4; 252 elements     (1, 64, 4)   exactly 256 elements
    (1, 257, 1)  B L = 1; 257 elements               (1, 65, 5)   B L = 5; text_len 0       (5, 130, 1)  B L = 5 over utterances
    (2, 130, 7)  accumulate 0 into NaN, accumulate 1 onto seeded values; NaN-filled workspace; a short one is refused with -2

Tolerances.  Exact where the arithmetic is exact: pad_rows (fp32, bf16, the hi plane), masked and padded zeros, dSt against dS, the
accumulating sum.  Otherwise max |diff| / max |ref| against float64: the same formula evaluated in fp32 torch on the CPU at every
case above loses the figure below (max over the cases; re-measured and printed per case by
test_aligner_reference_host.py::test_fp32_noise_table; recorded 1.4 x above the measurement, see there), and the kernel is
allowed 8 x that, capped at 1e-4.

    output                      fp32 noise   tolerance
    instnorm out                2.2e-7       1.76e-6     (bf16: + 2^-8 max(1, |ref|); split: + 2^-21 |ref| + 2^-24, per element)
    instnorm_bwd d_y            1.0e-6       8.00e-6
    instnorm_bwd d_weight       2.8e-7       2.24e-6
    instnorm_bwd d_bias         3.0e-7       2.40e-6
    scores logits               1.1e-6       8.80e-6
    scores soft                 1.9e-6       1.52e-5     (the figure comes from (2, 64, 64), whose scores reach 80)
    scores_bwd dS               4.8e-7       3.84e-6     (L = 1: the unit is scale max |cotangent|, the reference being 0)
    soft_average_bwd dA         7.9e-7       6.32e-6

The prior's cutoff.  A cell whose float64 prior is within 1e-4 (relative) of 1e-4 may fall on either side in fp32 (the fp32 prior
is 2.7e-6 from float64, the band 37 x that): the comparison leaves such a cell out of `logits` and its row out of `soft` and `dS`.
That is one row each of (2, 130, 289) and (3, 65, 320) and none elsewhere (asserted on the CPU by test_prior_cutoff_band).

The fast path's bound (derived, aligner_reference.fast_logit_bound; proved on the CPU by test_fast_path_bound: the three-term
emulation stays inside, an emulation that loses a cross term leaves it by 45 x or more)
    |logit - ref| <= fp32 tolerance * max |ref|  +  2 * 2^-16 * scale * (|q_m| . |k_j| + max_j' |q_m| . |k_j'|)  +  T
  product term: each operand is hi + lo with hi = bf16(v), lo = bf16(v - hi), 16 significant bits: |v - hi - lo| <= 2^-17 |v|; the
  dropped lo.lo is below 2^-16 |q| |k| ... 2^-18; together under 2 * 2^-16 |q_m| . |k_j| for score (m, j); the row's log-sum-exp
  moves by at most the largest score error of the row, the second summand.
  T, the transcendentals: exp(x) is v_exp_f32(x * log2e): the product's rounding and the constant's move the exponent by at most
  2^-23 |x| log2e, the result by the factor 2^-23 |x|, and v_exp_f32 is good to 1 ulp: e(x) = 2^-23 (1 + |x|) relative.  log(y) is
  v_log_f32(y) * ln2: 1 ulp, the product's rounding and the constant's: 2^-22 |log y| absolute.  So the log-sum-exp carries
  e(A) + 2^-22 log L with A = max |s - rowmax| of the case (160 where the scores reach +-80), and log(prior + 1e-6), a quotient of
  exponentials with |x| < 50 under a logarithm of at most log 1e6, carries 2 e(50) + 2^-22 * 13.82:
  T = e(A) + 2 e(50) + 2^-22 (log L + 13.82), 1.6e-5 to 2.8e-5 over the cases.
    |soft - ref| <= fp32 tolerance + 2 * (the row's largest logit bound)          (d softmax <= 2 max |d logit|)
"""
import pytest
import torch

import aligner_reference as R
from isp_tts_amd import runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
NAN = float("nan")


def _dev(t):
    return None if t is None else t.to(DEV)


def _unchanged(pairs):
    for name, d, h in pairs:
        assert d is None or R.same_bits(d, h), f"{name} was written"


def _max0(t) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


def _nan_workspace(floats):
    """The workspace the wrappers will take on this stream, NaN-filled."""
    runtime.workspace(DEV, floats).fill_(NAN)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ pad_rows


@pytest.mark.parametrize("mode,out_dtype", R.PAD_MODES)
@pytest.mark.parametrize("case", list(R.PAD_CASES))
def test_pad_rows(case, mode, out_dtype):
    B, T, C = case
    i = R.pad_inputs(case)
    x_h = R.pad_view(i["base"], case)[2]
    base, lens = i["base"].to(DEV), i["lengths"].to(DEV)
    x, channel_first, _ = R.pad_view(base, case)
    if R.PAD_CASES[case] == "cf":
        assert x.stride(2) == 1 and x.stride(1) == T + 3          # the tile kernel's condition, but for B
    run = lambda: runtime.pad_rows(x, lens, channel_first=channel_first, out_dtype=out_dtype).cpu()      # noqa: E731
    got = run()
    want = R.pad_rows_ref(x_h, i["lengths"], mode, dtype=F32)
    assert got.dtype == out_dtype and got.shape == want.shape
    if mode == "split":
        assert R.same_bits(got[0], want[0]), f"hi plane: {int((got[0] != want[0]).sum())} values differ from fp16(clamp(x))"
        assert bool(torch.isfinite(got).all())
        v = R.pad_rows_ref(x_h, i["lengths"])
        err = (got[0].double() + got[1].double() - v.clamp(-R.SPLIT_MAX, R.SPLIT_MAX)).abs()
        assert bool((err <= R.split_bound(v)).all()), f"hi + lo: worst |diff| / bound = {float((err / R.split_bound(v)).max()):.3f}"
    else:
        assert torch.equal(got, want), f"{int((got != want).sum())} values differ"
    assert R.same_bits(run(), got)
    _unchanged([("x", base, i["base"]), ("lengths", lens, i["lengths"])])


# ------------------------------------------------------------------------------------------------ masked instance norm


@pytest.mark.parametrize("mode,out_dtype", R.INSTNORM_MODES)
@pytest.mark.parametrize("case", list(R.INSTNORM_CASES))
def test_masked_instnorm(case, mode, out_dtype):
    B, T, C = case
    i = R.instnorm_inputs(case)
    want = R.masked_instnorm_ref(**i)
    d = {k: i[k].to(DEV) for k in ("y", "weight", "bias", "lengths")}
    run = lambda: runtime.masked_instnorm(d["y"], d["weight"], d["bias"], d["lengths"], out_dtype=out_dtype).cpu()      # noqa: E731
    got = run()
    assert got.dtype == out_dtype and got.shape == ((2, B, T + 4, C) if mode == "split" else (B, T + 4, C))
    assert bool(torch.isfinite(got).all()), "a NaN of the rows t >= n reached the output"
    val = got[0].double() + got[1].double() if mode == "split" else got.double()
    tol = R.tol("instnorm.out")
    print(f"{case} {mode}: max |diff| / max |ref| = {R.rel_err(val, want):.3e} (fp32 tolerance {tol:.3g})")
    if mode == "f32":
        R.close(val, want, tol, "out")
    else:
        extra = 2.0 ** -8 * want.abs().clamp(min=1.0) if mode == "bf16" else R.split_bound(want)
        err, bound = (val - want).abs(), tol * float(want.abs().max()) + extra
        assert bool((err <= bound).all()), f"worst |diff| / bound = {float((err / bound).max()):.3f}"
    n = i["lengths"].clamp(1, T)
    planes = got if mode == "split" else got[None]
    for b in range(B):
        nb = int(n[b])
        assert _max0(planes[:, b, :2]) == 0.0 and _max0(planes[:, b, nb + 2:]) == 0.0, f"utterance {b}: a padding row is not zero"
        if nb == 1 and mode == "f32":
            assert torch.equal(got[b, 2], i["bias"]), "n = 1: the output is not exactly bias"
    assert R.same_bits(run(), got)
    _unchanged([(k, d[k], i[k]) for k in d])


@pytest.mark.parametrize("case", list(R.INSTNORM_BWD_CASES))
def test_masked_instnorm_bwd(case):
    B, T, C = case
    i = R.instnorm_inputs(case, backward=True)
    want = R.masked_instnorm_bwd_ref(i["y"], i["d_out"], i["weight"], i["lengths"])
    d = {k: i[k].to(DEV) for k in ("y", "d_out", "weight", "lengths")}

    def run():
        _nan_workspace(2 * B * C)
        return [t.cpu() for t in runtime.masked_instnorm_bwd(d["y"], d["d_out"], d["weight"], d["lengths"])]
    got = run()
    n = i["lengths"].clamp(1, T)
    for name, g, w in zip(("d_y", "d_weight", "d_bias"), got, want):
        print(f"{case} {name}: {R.rel_err(g, w):.3e} (tolerance {R.tol('instnorm_bwd.' + name):.3g})")
    for name, g, w in zip(("d_y", "d_weight", "d_bias"), got, want):
        assert g.dtype == F32 and bool(torch.isfinite(g).all()), f"{name} is not finite"
        R.close(g, w, R.tol(f"instnorm_bwd.{name}"), name)
    for b in range(B):
        assert _max0(got[0][b, int(n[b]):]) == 0.0, f"utterance {b}: d_y is not zero in the rows t >= n"
    for a, b in zip(run(), got):
        assert R.same_bits(a, b)
    _unchanged([(k, d[k], i[k]) for k in d])


def test_masked_instnorm_bwd_refusals():
    """A workspace shorter than 2 B C floats: -2; a NULL pointer: -1.  Nothing is launched: the outputs keep their NaN."""
    B, T, C = 2, 9, 260
    i = R.instnorm_inputs((B, T, C), backward=True)
    y, d_out, w, lens = (i[k].to(DEV) for k in ("y", "d_out", "weight", "lengths"))
    d_y, dw, db = torch.full_like(y, NAN), torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    ws = torch.full((2 * B * C,), NAN, device=DEV)
    fn = runtime.lib().ispk_masked_instnorm_bwd_f32
    args = lambda y_ptr, floats: (y_ptr, d_out.data_ptr(), w.data_ptr(), lens.data_ptr(), d_y.data_ptr(), dw.data_ptr(),      # noqa: E731
                                  db.data_ptr(), ws.data_ptr(), floats, B, T, C, 1e-5, _stream())
    assert fn(*args(y.data_ptr(), 2 * B * C - 1)) == -2
    assert fn(*args(None, 2 * B * C)) == -1
    torch.cuda.synchronize()
    for t in (d_y, dw, db, ws):
        assert bool(torch.isnan(t).all())
    assert fn(*args(y.data_ptr(), 2 * B * C)) == 0 and bool(torch.isfinite(dw).all())


# ------------------------------------------------------------------------------------------------ scores


def _scores_device(i):
    wide = _dev(i["wide"])
    q = wide[::2] if wide is not None else i["q"].to(DEV)
    held = [("q", wide if wide is not None else q, i["wide"] if wide is not None else i["q"])]
    k, tl, ml = i["k"].to(DEV), i["text_len"].to(DEV), i["mel_len"].to(DEV)
    return q, k, tl, ml, held + [("k", k, i["k"]), ("text_len", tl, i["text_len"]), ("mel_len", ml, i["mel_len"])]


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("case", list(R.SCORES_CASES))
def test_aligner_scores(case, fast):
    B, M, L = case
    i = R.scores_inputs(case)
    want_soft, want_logits = R.aligner_scores_ref(i["q"], i["k"], i["text_len"], i["mel_len"], M, L)
    q, k, tl, ml, held = _scores_device(i)
    if case == R.SCORES_Q_SLICE:
        assert q.stride(0) == 2 * (M + 4) * R.AD
    run = lambda: [t.cpu() for t in runtime.aligner_scores(q, k, tl, ml, M, L, fast=fast)]      # noqa: E731
    soft, logits = run()
    assert soft.shape == logits.shape == (B, M, L) and soft.dtype == logits.dtype == F32
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(soft).all()), "a stored value is NaN or infinite"
    cells, rows = R.scores_checked(case)
    live = R.live_rows(case)
    tlc, lt, st = i["text_len"].clamp(1, L), R.tol("scores.logits"), R.tol("scores.soft")
    dead = (torch.arange(L)[None, None, :] >= tlc[:, None, None]) | ~live[:, :, None]
    assert _max0(soft[dead.expand(B, M, L)]) == 0.0, "soft is not exactly 0 behind text_len or mel_len"
    print(f"{case} {'fast' if fast else 'exact'}: logits {R.rel_err(logits[cells], want_logits[cells]):.3e} (fp32 tolerance {lt:.3g}), "
          f"soft {R.rel_err(soft[rows], want_soft[rows]):.3e} ({st:.3g})")
    if fast:
        bound = R.fast_logit_bound(i["q"], i["k"], M, L, lt * float(want_logits[cells].abs().max()))
        err = (logits.double() - want_logits).abs()
        print(f"    logits: worst |diff| / bound = {float((err / bound)[cells].max()):.3f}")
        assert bool((err <= bound)[cells].all()), f"logits: worst |diff| / bound = {float((err / bound)[cells].max()):.3f}"
        sbound = (st + 2 * bound.max(-1, keepdim=True).values).expand(B, M, L)
        serr = (soft.double() - want_soft).abs()
        print(f"    soft: worst |diff| / bound = {float((serr / sbound)[rows].max()):.3f}")
        assert bool((serr <= sbound)[rows].all()), f"soft: worst |diff| / bound = {float((serr / sbound)[rows].max()):.3f}"
    else:
        R.close(logits[cells], want_logits[cells], lt, "logits")
        R.close(soft[rows], want_soft[rows], st, "soft")
    sums = soft.double().sum(-1)[live]
    assert float((sums - 1.0).abs().max()) <= st, f"a live row of soft sums to 1 +- {float((sums - 1.0).abs().max()):.3e}"
    for a, b in zip(run(), (soft, logits)):
        assert R.same_bits(a, b)
    _unchanged(held)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_aligner_scores_refusals(fast):
    """L = 321: -2; D = 64: -4; q four bytes off a 16-byte boundary: -3.  Nothing is launched: the outputs keep their NaN."""
    B, M, L = 2, 5, 321
    q, k = torch.zeros((B, M + 4, 128), device=DEV), torch.zeros((B, L + 4, 128), device=DEV)
    tl, ml = torch.tensor([L, 3], device=DEV), torch.tensor([M, 2], device=DEV)
    logits, soft = torch.full((B, M, L), NAN, device=DEV), torch.full((B, M, L), NAN, device=DEV)
    fn = runtime.lib().ispk_aligner_scores_fast_f32 if fast else runtime.lib().ispk_aligner_scores_f32
    call = lambda q_ptr, L_, D_: fn(q_ptr, q.stride(0), k.data_ptr(), k.stride(0), tl.data_ptr(), ml.data_ptr(), logits.data_ptr(),      # noqa: E731
                                    soft.data_ptr(), B, M, L_, D_, _stream())
    assert call(q.data_ptr(), 321, 128) == -2
    assert call(q.data_ptr(), 320, 64) == -4
    assert call(q.data_ptr() + 4, 320, 128) == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(soft).all())


@pytest.mark.parametrize("mode", R.SCORES_BWD_MODES)
@pytest.mark.parametrize("case", list(R.SCORES_BWD_CASES))
def test_aligner_scores_bwd(case, mode):
    B, M, L = case
    i = R.scores_bwd_inputs(case, mode)
    keys = ("logits", "soft", "d_soft", "d_logits", "text_len", "mel_len")
    want = R.aligner_scores_bwd_ref(*(i[k] for k in keys))
    d = {k: _dev(i[k]) for k in keys}
    run = lambda: [t.cpu() for t in runtime.aligner_scores_bwd(*(d[k] for k in keys), R.SCALE)]      # noqa: E731
    dS, dSt = run()
    L4, M4 = (L + 3) // 4 * 4, (M + 3) // 4 * 4
    assert dS.shape == (B, M, L4) and dSt.shape == (B, L, M4) and dS.dtype == dSt.dtype == F32
    assert torch.equal(dSt[:, :, :M].view(torch.int32), dS[:, :, :L].transpose(1, 2).view(torch.int32)), "dSt is not the transposed copy of dS"
    assert _max0(dS[:, :, L:]) == 0.0 and _max0(dSt[:, :, M:]) == 0.0, "a padding column was written"
    assert bool(torch.isfinite(dS).all())
    _, rows = R.scores_checked(case, R.SCORES_BWD_CASES)
    e = R.scores_bwd_err(dS[:, :, :L][rows], want[rows], i)
    print(f"{case} {mode}: dS {e:.3e} (tolerance {R.tol('scores_bwd.dS'):.3g})")
    assert e <= R.tol("scores_bwd.dS"), f"dS: {e:.3e}"
    if mode == "soft":
        assert _max0(dS[~R.live_rows(case, R.SCORES_BWD_CASES)]) == 0.0, "a row past mel_len has gradient without d_logits"
    for a, b in zip(run(), (dS, dSt)):
        assert R.same_bits(a, b)
    _unchanged([(k, d[k], i[k]) for k in keys])


def test_aligner_scores_bwd_refuses_two_null_cotangents():
    B, M, L = 1, 5, 65
    i = R.scores_bwd_inputs((B, M, L), "both")
    logits, soft, tl, ml = (i[k].to(DEV) for k in ("logits", "soft", "text_len", "mel_len"))
    dS, dSt = torch.full((B, M, 68), NAN, device=DEV), torch.full((B, L, 8), NAN, device=DEV)
    rc = runtime.lib().ispk_aligner_scores_bwd_f32(logits.data_ptr(), soft.data_ptr(), None, None, tl.data_ptr(), ml.data_ptr(),
                                                   dS.data_ptr(), 68, dSt.data_ptr(), 8, B, M, L, R.SCALE, _stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool(torch.isnan(dS).all()) and bool(torch.isnan(dSt).all())


# ------------------------------------------------------------------------------------------------ soft averages, backward


@pytest.mark.parametrize("case", list(R.SA_BWD_CASES))
def test_soft_average_bwd(case):
    B, M, L = case
    i = R.sa_bwd_inputs(case)
    keys = ("attn", "pitch", "energy", "d_feats", "text_len")
    want = R.soft_average_bwd_ref(*(i[k] for k in keys))
    d = {k: i[k].to(DEV) for k in keys}

    def run(prior=None):
        _nan_workspace(3 * B * L)
        out = torch.full((B, M, L), NAN, device=DEV) if prior is None else prior.to(DEV)
        got = runtime.soft_average_bwd(*(d[k] for k in keys), out=out, accumulate=prior is not None)
        assert got.data_ptr() == out.data_ptr()
        return got.cpu()
    got = run()
    assert got.dtype == F32 and bool(torch.isfinite(got).all()), "the NaN of the output or the workspace survived"
    print(f"{case}: dA {R.rel_err(got, want):.3e} (tolerance {R.tol('soft_average_bwd.dA'):.3g})")
    if float(want.abs().max()) == 0.0:
        assert _max0(got) == 0.0
    else:
        R.close(got, want, R.tol("soft_average_bwd.dA"), "dA")
    masked = (torch.arange(L)[None] >= i["text_len"][:, None])[:, None, :].expand(B, M, L)
    assert _max0(got[masked]) == 0.0, "a masked column has gradient"
    acc = run(i["prior"])
    assert R.same_bits(acc, i["prior"] + got), "accumulate = 1 is not the fp32 sum of the prior value and the accumulate = 0 result"
    assert R.same_bits(run(), got) and R.same_bits(run(i["prior"]), acc)
    assert R.same_bits(runtime.soft_average_bwd(*(d[k] for k in keys)).cpu(), got), "the defaults do not give the accumulate = 0 result"
    _unchanged([(k, d[k], i[k]) for k in keys])


def test_soft_average_bwd_refuses_a_short_workspace():
    B, M, L = 2, 130, 7
    i = R.sa_bwd_inputs((B, M, L))
    attn, pitch, energy, g, tl = (i[k].to(DEV) for k in ("attn", "pitch", "energy", "d_feats", "text_len"))
    ws, out = torch.full((3 * B * L,), NAN, device=DEV), torch.full((B, M, L), NAN, device=DEV)
    fn = runtime.lib().ispk_soft_average_bwd_f32
    call = lambda floats: fn(attn.data_ptr(), pitch.data_ptr(), energy.data_ptr(), g.data_ptr(), tl.data_ptr(), ws.data_ptr(), floats,      # noqa: E731
                             out.data_ptr(), 0, B, M, L, _stream())
    assert call(3 * B * L - 1) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())
    assert call(3 * B * L) == 0 and bool(torch.isfinite(out).all())
