"""The in-kernel dropout and the GELU pair against a host model (tests/dropout_reference.py, itself checked by
tests/test_dropout_host.py): every mask comes from the host mirror of csrc/dropout.h, every value from float64 with the exact erf -
no kernel of this project is the reference of another here.

  * ispk_dropout_mask_u8 bit for bit, over sizes around the 256-thread block, the edges of p, seeds with high bits, the seed source's
    words, and seeds built so that an element's hash sits exactly on / one below the threshold (keep is `>=`);
  * the six element-wise entry points (ispk_gelu_f32 / _f32_bf16 / _bf16, ispk_gelu_bwd_f32 / _bf16 / _b16) over EVERY finite bf16
    input up to 2^64 and, for the fp32-input forms, fp32 values that are no bf16 numbers;
  * the two GEMM epilogues (ISPK_EP_DUAL_GELU, ISPK_EP_GELU_BWD) with exact pre-activations from a selector operand, at a row tail,
    a partial column tile (N % 64 != 0), both panel depths, and leading dimensions wider than N.

The rule for every output element (`s` = 1 / (1 - p) as the launchers compute it, times |da| for a backward):
  * dropped by the mirror -> exactly 0;
  * |got - ref| <= bound, per element - never max error over max magnitude;
  * kept with |ref| > bound -> nonzero (which the line above implies; stated because it replaces an "almost equal masks" escape).
bound, bf16 outputs: 2^-8 |ref| (one bf16 rounding, with room) + EPS_FAST s max(|u|, 1) forward, + EPS_FAST s backward; EPS_FAST is
derived on the host (dropout_reference.py).  Plus 2^-134, half the spacing of bf16's denormals, where the relative term stops
describing a rounding: the epilogue tests take da from the grid, denormals included, and du = da gelu'(u) then lands between two
denormals with nothing else in the bound (the kernels round those correctly, ties to even).
bound, fp32 forms (device libm erff / expf): twice the error measured on an MI355X, recorded below, and never above the bars
tests/test_gpu_train.py::test_gelu_forward_backward has always held them to."""
import functools

import numpy as np
import pytest
import torch

import dropout_reference as dr
from isp_tts_amd import runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"

# max |err| / (s max(|u|, 1)) of ispk_gelu_f32 and max |err| / s of ispk_gelu_bwd_f32 against float64 over every case of
# test_gelu_forward_forms_ / test_gelu_backward_forms_match_float64 (which print them), measured on an MI355X (gfx950) on 2026-10-20 with the kernels of commit
# 69bd09f (the change that added this file alters none): 1.399e-7 and 1.777e-7, both on the fp32 linspace input at p = 0.1.  The
# tests assert twice these: room for libm differences between ROCm point releases.
F32_FWD_MEASURED = 1.4e-7
F32_BWD_MEASURED = 1.8e-7
F32_FWD_BAR, F32_BWD_BAR = 1e-6, 2e-6          # the project's bars for the fp32 pair: asserted bounds may not exceed them

MASK_NS = (1, 255, 256, 257, 65539)
MASK_PS = (0.0, 1e-12, 0.1, 0.3, 0.5, 0.999, float(np.nextafter(np.float32(1), np.float32(0))))
MASK_SEEDS = (0, 1, 1234, 2 ** 63 + 12345, 2 ** 64 - 1)
WORDS = (0, 1, 2, -1, 2 ** 62)
CASES = ((0.0, 0), (0.1, 1234), (0.5, 2 ** 63 + 7))
FWD_FORMS = (("ispk_gelu_f32", torch.float32, torch.float32), ("ispk_gelu_f32_bf16", torch.float32, torch.bfloat16),
             ("ispk_gelu_bf16", torch.bfloat16, torch.bfloat16))
BWD_FORMS = (("ispk_gelu_bwd_f32", torch.float32, torch.float32), ("ispk_gelu_bwd_bf16", torch.float32, torch.bfloat16),
             ("ispk_gelu_bwd_b16", torch.bfloat16, torch.bfloat16))          # (entry, u's type, da / du's type)
BF16_HALF_DENORMAL = 2.0 ** -134                # half the spacing of bf16's denormals (2^-133)
SENTINEL = 0x7FC1                               # a bf16 NaN pattern no kernel here produces


class Source:
    """`with Source(word):` sets the dropout seed source to a device word holding `word` (None: leaves it unset)."""

    def __init__(self, word):
        self.word = word

    def __enter__(self):
        if self.word is not None:
            w = self.word - 2 ** 64 if self.word >= 2 ** 63 else self.word
            self.t = torch.tensor([w], dtype=torch.int64, device=DEV)
            runtime.set_seed_source(self.t)

    def __exit__(self, *exc):
        runtime.set_seed_source(None)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the mask kernel
def _host_masks(p, word):
    return {seed: dr.keep_mask(seed, max(MASK_NS), p, word) for seed in MASK_SEEDS}


def _assert_masks(p, word):
    for seed, want in _host_masks(p, word).items():
        for n in MASK_NS:
            got = runtime.dropout_mask(n, p, seed, DEV).cpu().numpy()
            assert np.array_equal(got, want[:n]), (f"p={p!r} seed={seed} n={n} word={word}: {int((got != want[:n]).sum())} of {n} "
                                                   f"keep decisions differ from the host mirror")


@pytest.mark.parametrize("p", MASK_PS)
def test_mask_equals_the_host_mirror(p):
    _assert_masks(p, None)
    if p == 0.0:
        assert bool(runtime.dropout_mask(257, p, 5, DEV).all())
    if p == 1e-12:                      # threshold 1, not 0: dropout is ON and drops the one hash value 0
        seed = dr.seed_for_hash(200, 0)
        got = runtime.dropout_mask(257, p, seed, DEV).cpu().numpy()
        assert not got[200] and got.sum() == 256


def test_mask_under_the_seed_source():
    base = runtime.dropout_mask(65539, 0.3, 1234, DEV)
    try:
        for word in WORDS:
            with Source(word):
                for p in MASK_PS:
                    _assert_masks(p, word)
    finally:
        runtime.set_seed_source(None)
    assert torch.equal(runtime.dropout_mask(65539, 0.3, 1234, DEV), base)
    assert np.array_equal(base.cpu().numpy(), dr.keep_mask(1234, 65539, 0.3))


@pytest.mark.parametrize("p", MASK_PS[1:])
def test_mask_threshold_boundary(p):
    """keep is hash >= thresh with thresh from the FLOAT p: a seed under which element idx hashes to exactly thresh keeps it, one
    under which it hashes to thresh - 1 drops it.  (Random seeds meet such a hash once in 2^32 elements.)"""
    t = dr.drop_thresh(p)
    for idx in (0, 255, 256, 65538):
        for value, keep in ((t, True), (t - 1, False), (2 ** 32 - 1, True), (0, False)):
            seed = dr.seed_for_hash(idx, value)
            got = runtime.dropout_mask(65539, p, seed, DEV).cpu().numpy()
            assert bool(got[idx]) == keep, f"p={p!r}: element {idx} with hash {value} against threshold {t}"
            assert np.array_equal(got, dr.keep_mask(seed, 65539, p))


# ------------------------------------------------------------------------------------------------ element-wise forms
@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> (u fp32 CPU tensor, gelu(u), gelu'(u) in float64, da fp32 CPU tensor): computed once, never modified."""
    grid = dr.finite_bf16_grid().float()
    lin = torch.linspace(-12.0, 12.0, 4 * 4099, dtype=torch.float64).float()
    assert float((lin.bfloat16().float() != lin).float().mean()) > 0.98
    # gelu' changes sign at u = -0.75179..: within 2e-4 of it |gelu'| < 1e-4, the relative part of the bound vanishes and
    # EPS_FAST alone is left - the sharpest look at gelu_grad_fast that a bf16 output allows
    cross = torch.linspace(-0.7518 - 2e-4, -0.7518 + 2e-4, 4 * 1001, dtype=torch.float64).float()
    out = {}
    for k, (name, u) in enumerate((("grid", grid), ("linspace", lin), ("crossing", cross))):
        u64 = u.double().numpy()
        da = torch.randn(u.shape, generator=torch.Generator().manual_seed(4000 + k))
        out[name] = (u, dr.gelu(u64), dr.gelu_grad(u64), da)
    return out


def _assert_rule(got, ref, keep, bound, what):
    got = got.double().cpu().numpy()
    assert not got[~keep].any(), f"{what}: {int((got[~keep] != 0).sum())} dropped elements are not exactly 0"
    err = np.abs(got - ref)
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (f"{what}: {int((err > bound).sum())} elements over the bound; worst at {worst}: got {got.flat[worst]!r}, "
                                  f"want {ref.flat[worst]!r}, bound {bound.flat[worst]:.3e}")
    must = keep & (np.abs(ref) > bound)
    assert got[must].all(), f"{what}: {int((got[must] == 0).sum())} kept elements with |ref| over the bound are 0"


def _forward_case(entry, ut, ot, name, p, seed, word=None):
    u, g64, _, _ = _inputs()[name]
    n, s = u.numel(), dr.inv_keep(p)
    keep = dr.keep_mask(seed, n, p, word)
    ref = g64 * keep * s
    scale = s * np.maximum(np.abs(u.double().numpy()), 1.0)
    got = runtime.gelu(u.to(ut).to(DEV), p, seed, out_dtype=ot)
    assert got.dtype == ot
    what = f"{entry}({name}, p={p}, seed={seed}, word={word})"
    if ot == torch.bfloat16:
        _assert_rule(got, ref, keep, 2.0 ** -8 * np.abs(ref) + BF16_HALF_DENORMAL + dr.EPS_FAST * scale, what)
        return None
    figure = float((np.abs(got.double().cpu().numpy() - ref) / scale).max())
    print(f"{what}: max |err| / (s max(|u|, 1)) = {figure:.3e}")
    _assert_rule(got, ref, keep, 2 * F32_FWD_MEASURED * scale, what)
    return figure


def _backward_case(entry, ut, dt, name, p, seed, word=None):
    u, _, d64, da = _inputs()[name]
    n, s = u.numel(), dr.inv_keep(p)
    keep = dr.keep_mask(seed, n, p, word)
    da = da.to(dt)
    da64 = da.double().numpy()
    ref = da64 * d64 * keep * s
    scale = s * np.abs(da64)
    ud, dad = u.to(ut).to(DEV), da.to(DEV)
    got = runtime.gelu_bwd(dad, ud, dropout_p=p, seed=seed)
    assert got.dtype == dt
    what = f"{entry}({name}, p={p}, seed={seed}, word={word})"
    figure = None
    if dt == torch.bfloat16:
        _assert_rule(got, ref, keep, 2.0 ** -8 * np.abs(ref) + BF16_HALF_DENORMAL + dr.EPS_FAST * scale, what)
    else:
        figure = float((np.abs(got.double().cpu().numpy() - ref) / scale).max())
        print(f"{what}: max |err| / s = {figure:.3e}")
        _assert_rule(got, ref, keep, 2 * F32_BWD_MEASURED * scale, what)
    # the aliasing train/stack.py uses: du written over da
    alias = dad.clone()
    assert runtime.gelu_bwd(alias, ud, out=alias, dropout_p=p, seed=seed) is alias
    assert torch.equal(alias.view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                       got.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), f"{what}: out=da differs from out of place"
    return figure


def test_the_recorded_fp32_figures_respect_the_bars():
    assert 2 * F32_FWD_MEASURED <= F32_FWD_BAR and 2 * F32_BWD_MEASURED <= F32_BWD_BAR


@pytest.mark.parametrize("p,seed", CASES)
@pytest.mark.parametrize("entry,ut,ot", FWD_FORMS)
def test_gelu_forward_forms_match_float64(entry, ut, ot, p, seed):
    for name in ("grid", "linspace", "crossing") if ut == torch.float32 else ("grid",):
        _forward_case(entry, ut, ot, name, p, seed)


@pytest.mark.parametrize("p,seed", CASES)
@pytest.mark.parametrize("entry,ut,dt", BWD_FORMS)
def test_gelu_backward_forms_match_float64(entry, ut, dt, p, seed):
    for name in ("grid", "linspace", "crossing") if ut == torch.float32 else ("grid",):
        _backward_case(entry, ut, dt, name, p, seed)


def test_elementwise_forms_at_the_threshold():
    """The six forms evaluate the same `>=` on the same index: element idx of a vector of ones is kept when its hash equals the
    threshold and dropped one below it."""
    n, p = 1028, 0.3
    t = dr.drop_thresh(p)
    for idx in (0, 3, 1023, 1026):                       # both ends of a thread's four lanes, the last full and the partial block
        for value, keep in ((t, True), (t - 1, False)):
            seed = dr.seed_for_hash(idx, value)
            want = dr.keep_mask(seed, n, p)
            assert bool(want[idx]) == keep
            for entry, ut, ot in FWD_FORMS:
                got = runtime.gelu(torch.ones(n, dtype=ut, device=DEV), p, seed, out_dtype=ot)
                assert np.array_equal((got != 0).cpu().numpy(), want), (entry, idx, value)
            for entry, ut, dt in BWD_FORMS:
                got = runtime.gelu_bwd(torch.ones(n, dtype=dt, device=DEV), torch.ones(n, dtype=ut, device=DEV), dropout_p=p, seed=seed)
                assert np.array_equal((got != 0).cpu().numpy(), want), (entry, idx, value)


# ------------------------------------------------------------------------------------------------ the two GEMM epilogues
def _grid_fill(N, K, mul, add):
    g = dr.finite_bf16_grid()
    i = (torch.arange(N * K, dtype=torch.int64) * mul + add) % g.numel()
    return g[i].view(N, K).contiguous()


class Wide:
    """An [M, N] bf16 matrix with leading dimension ld inside a buffer of M + 2 rows, every cell of which starts as SENTINEL."""

    def __init__(self, M, N, ld, fill=None):
        self.M, self.N, self.ld = M, N, ld
        self.buf = torch.full((M + 2, ld), SENTINEL, dtype=torch.int16, device=DEV)
        self.mat = self.buf.view(torch.bfloat16)[:M, :N]
        if fill is not None:
            self.mat.copy_(fill)

    def assert_outside_untouched(self, what):
        assert bool((self.buf[:self.M, self.N:] == SENTINEL).all()) and bool((self.buf[self.M:] == SENTINEL).all()), \
            f"{what}: a store outside [:, :N]"


def _gemm_gelu_train(x, w1, M, N, K, ld, p, seed):
    if ld == N:
        u, a = runtime.gemm_gelu_train(x, w1, p, seed)
        return u, a, None, None
    ub, ab = Wide(M, N, ld), Wide(M, N, ld)
    runtime._check(runtime.lib().ispk_gemm_bf16_gelu_train(x.data_ptr(), K, w1.data_ptr(), K, ub.mat.data_ptr(), ld, ab.mat.data_ptr(), ld,
                                                           M, N, K, p, seed, runtime._stream()), "ispk_gemm_bf16_gelu_train")
    return ub.mat, ab.mat, ub, ab


def _gemm_gelu_bwd(dy, w2t, u, mask, M, N, K, ld, p, seed):
    if ld == N:
        return runtime.gemm_gelu_bwd(dy, w2t, u, mask, p, seed), None
    ub, db = Wide(M, N, ld, fill=u), Wide(M, N, ld)
    runtime._check(runtime.lib().ispk_gemm_bf16_gelu_bwd(dy.data_ptr(), K, w2t.data_ptr(), K, ub.mat.data_ptr(), ld, db.mat.data_ptr(), ld,
                                                         None if mask is None else mask.data_ptr(), M, N, K, p, seed, runtime._stream()),
                   "ispk_gemm_bf16_gelu_bwd")
    ub.assert_outside_untouched("u of gemm_gelu_bwd (an input)")
    return db.mat, db


def _epilogue_case(M, N, K, strided, p, seed, word=None):
    ld = N + 8 if strided else N
    w1, w2t = _grid_fill(N, K, 1, 0), _grid_fill(N, K, 31, 17)
    r = torch.arange(M)
    sel = torch.zeros(M, K, dtype=torch.bfloat16)
    sel[r, r % K] = 1.0
    want_u, want_da = w1[:, r % K].t().contiguous(), w2t[:, r % K].t().contiguous()          # [M, N]: exact products
    s = dr.inv_keep(p)
    keep = dr.keep_mask(seed, M * N, p, word).reshape(M, N)                                   # the mask index is m N + n, not m ld + n
    u64, da64 = want_u.double().numpy(), want_da.double().numpy()
    what = f"M={M} N={N} K={K} ld={ld} p={p} word={word}"
    seld, w1d, w2d = sel.to(DEV), w1.to(DEV), w2t.to(DEV)

    u, a, ub, ab = _gemm_gelu_train(seld, w1d, M, N, K, ld, p, seed)
    assert torch.equal(u.cpu(), want_u), f"{what}: u is not the selected weights"
    same = (want_u.view(torch.int16) != -32768)                                                # (-0 + 0 = +0 in the accumulator)
    assert torch.equal(u.cpu().view(torch.int16)[same], want_u.view(torch.int16)[same]), f"{what}: u differs in its bits"
    ref = dr.gelu(u64) * keep * s
    _assert_rule(a, ref, keep, 2.0 ** -8 * np.abs(ref) + BF16_HALF_DENORMAL + dr.EPS_FAST * s * np.maximum(np.abs(u64), 1.0), f"a, {what}")
    for b, name in ((ub, "u"), (ab, "a")):
        if b is not None:
            b.assert_outside_untouched(f"{name}, {what}")

    for masked in (False, True):
        rows = (r % 7 != 3) if masked else torch.ones(M, dtype=torch.bool)
        du, db = _gemm_gelu_bwd(seld, w2d, want_u.to(DEV), rows.to(DEV) if masked else None, M, N, K, ld, p, seed)
        d64 = da64 * rows.numpy()[:, None]
        ref = d64 * dr.gelu_grad(u64) * keep * s
        kept = keep & rows.numpy()[:, None]
        _assert_rule(du, ref, kept, 2.0 ** -8 * np.abs(ref) + BF16_HALF_DENORMAL + dr.EPS_FAST * s * np.abs(d64), f"du (masked={masked}), {what}")
        if db is not None:
            db.assert_outside_untouched(f"du, {what}")


@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("strided", (False, True))
@pytest.mark.parametrize("M,N,K", [(293, 256, 256), (293, 200, 256), (70, 264, 384)])
def test_gemm_epilogues_match_float64(M, N, K, strided, p):
    _epilogue_case(M, N, K, strided, p, 2 ** 63 + 99)


# ------------------------------------------------------------------------------------------------ one seed word, every kernel form
def test_seed_source_gives_every_form_the_same_mask():
    """With one word set, the six element-wise forms and both epilogues drop exactly the elements keep_mask(seed, n, p, word) drops:
    forward and backward agree on every element, not on almost all."""
    word, p, seed = 0x0123456789ABCDEF, 0.3, 77
    try:
        with Source(word):
            for entry, ut, ot in FWD_FORMS:
                _forward_case(entry, ut, ot, "grid", p, seed, word)
            for entry, ut, dt in BWD_FORMS:
                _backward_case(entry, ut, dt, "grid", p, seed, word)
            _epilogue_case(293, 200, 256, True, p, seed, word)
    finally:
        runtime.set_seed_source(None)
    _forward_case(*FWD_FORMS[0], "grid", p, seed, None)           # and without the source the plain mask is back
