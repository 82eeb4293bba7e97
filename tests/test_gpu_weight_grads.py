"""Weight-gradient reductions (ispk_gemm_tn_f32 / _bf16 / _b16 / _batched_f32, ispk_colsum_f32, ispk_smallk_wgrad_f32)
against float64, across the kernels behind gemm_tn_launch, its row-range plans, row masks and operand layouts.

Four kernels sit behind one launcher: gemm_tn_kernel (fp32, kernel 1), gemm_tn_bf16_kernel with fp32 operands rounded to
bf16 in flight (2) or bf16 operands staged through registers (3), and gemm_tn_dma_kernel (bf16 operands by LDS-DMA; no row
mask, batch 1, N1 and N2 multiples of 8: 4).  ispk_gemm_tn_last_plan reports which one ran and the plan (row ranges, rows
per range); a Python mirror of the planner (`_plan`) must agree with it for every case, and the shapes are chosen so that
every branch of the plan and of the kernels' XCD mapping is reached (test_planner_branches_are_all_reached), so a change of
the plan fails here instead of silently moving coverage elsewhere.

Main check - exactness on integer operands: A and B hold integers in [-4, 4] (masked rows of A: finite garbage +-2^20), so
every product and every partial sum is an integer below 2^24, exact in fp32 in any order, and the operands are exact in
bf16.  Every kernel, plan, mask, layout and accumulate case must then equal the float64 reference BIT FOR BIT: a dropped,
doubled or misplaced row, range, tile or column, or a mask leak, is an exact mismatch.  Rounding is checked separately on
normal operands (fp32: max |C - ref| <= 2e-6 max |ref|; bf16 paths against float64 over the RNE-rounded operands: 2e-5),
and at M = 1, where C is one outer product: bf16 products are exact in fp32, so the bf16 paths must equal the product of
the rounded operands bit for bit (this pins the in-flight rounding to RNE), and the fp32 path is within 1 ulp.

Every matrix case also checks that nothing outside C's view is written (C lives in a NaN-sentinel buffer with SLACK
elements after it), that operand padding is never read (it is NaN, which would reach C), and that a second call writes the
same bits.  Layouts: (a) contiguous; (b) A and B column slices of wider NaN-padded buffers; (c) C one element past an
aligned address; (d) ldc = N2 + 3; (e) B as overlapping windows (ldb < N2) built as aligner.py's _windows builds them;
(f) accumulate into a pre-filled C; (g) accumulate into a C with ldc > N2 at an offset (predictor.py's out=dw[:, k:]).

Masked rows: on the fp32 and bf16-in-flight paths A's masked rows are MULTIPLIED by zero; on the bf16-operand paths they
are SELECTED out (never loaded).  A non-finite value in a masked row of A therefore gives NaN on the first two paths and is
ignored on the others (B's rows are never masked on any path).  The garbage here is finite on purpose: that difference is
recorded behaviour, not something these tests change."""
import ctypes
import functools

import pytest
import torch

from isp_tts_amd import runtime

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLACK = 256                    # elements after every backing buffer: a stray store past the view lands inside it
NAN32 = 0x7FC0_1234            # sentinel bit patterns (quiet NaNs with a payload no kernel produces)
NAN16 = 0x7FC1
GARBAGE = float(2 ** 20)       # masked rows of A: large, finite, exact in bf16

F32, BF16, B16, DMA = 1, 2, 3, 4       # ispk_gemm_tn_last_plan's kernel ids


# --------------------------------------------------------------------------------------------- the planner's mirror
def _plan(M, N1, N2, batch, dma, ws_floats):
    """gemm_tn_launch's row-range plan -> (splits, rows_per); None where it refuses for the workspace."""
    tile = N1 * N2
    if ws_floats < tile * batch:
        return None
    tiles = -(-N1 // 128) * -(-N2 // 128) * batch
    target = 512 if dma else 1024
    splits = max(target // tiles, 1) if dma else -(-target // tiles)
    splits = min(splits, (M + 63) // 64, ws_floats // (tile * batch))
    splits = min(max(splits, 1), 256)
    rows_per = -(-M // splits)
    rows_per = -(-rows_per // 32) * 32
    return -(-M // rows_per), rows_per


def _branches(M, N1, N2, batch, kernel, splits, rows_per):
    """The plan / kernel branches a case reaches (for the coverage test and the failure messages)."""
    nz = splits * batch
    out = {f"k{kernel}"}
    if kernel in (BF16, B16, DMA):      # 1-D grids: the XCD mapping of row ranges
        out.add("nz<8" if nz < 8 else ("nz%8==0" if nz % 8 == 0 else "nz%8!=0"))
    if splits == 1:
        out.add("splits==1")
    out.add(f"chunks={min(rows_per // 32, 4)}")         # chunks of 32 rows in a full range (4: four or more)
    last = M - (splits - 1) * rows_per
    if last < rows_per:
        out.add("short-last")
        out.add(f"last-chunks={min(-(-last // 32), 4)}")
    return out


def _last_plan():
    s, r = ctypes.c_int32(-1), ctypes.c_int32(-1)
    k = runtime.lib().ispk_gemm_tn_last_plan(ctypes.byref(s), ctypes.byref(r))
    return k, s.value, r.value


def _err():
    s = runtime.lib().ispk_last_error_string()
    return s.decode() if s else ""


# --------------------------------------------------------------------------------------------- buffers
class Buf:
    """A flat device buffer filled with the sentinel and one strided 2-D view [rows, cols] of it at element offset `off`."""

    def __init__(self, dtype, rows, cols, ld, off=0, extra=0):
        self.dtype, self.rows, self.cols, self.ld, self.off = dtype, rows, cols, ld, off
        self.n = off + max(rows - 1, 0) * ld + cols + extra + SLACK
        self.flat = torch.empty(self.n, dtype=dtype, device=DEV)
        self.reset()

    @property
    def ints(self):
        return self.flat.view(torch.int16 if self.dtype == torch.bfloat16 else torch.int32)

    @property
    def sentinel(self):
        return NAN16 if self.dtype == torch.bfloat16 else NAN32

    def reset(self):
        self.ints.fill_(self.sentinel)

    @property
    def view(self):
        return torch.as_strided(self.flat, (self.rows, self.cols), (self.ld, 1), self.off)

    def ptr(self):
        return self.flat.data_ptr() + self.off * self.flat.element_size()

    def inside(self):
        keep = torch.zeros(self.n, dtype=torch.bool, device=DEV)
        torch.as_strided(keep, (self.rows, self.cols), (self.ld, 1), self.off).fill_(True)
        return keep

    def outside_touched(self, inside=None):
        """number of elements outside the view (or outside the given boolean element set) whose bits changed"""
        inside = self.inside() if inside is None else inside
        return int(((self.ints != self.sentinel) & ~inside).sum())


def _ints(shape, seed, lo=-4, hi=4):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV, dtype=torch.int32).float()


def _mask(kind, M):
    if kind is None:
        return None
    m = torch.arange(M, device=DEV)
    return {"ragged": (m % 5 != 2) & (m % 7 != 3), "none": torch.zeros(M, dtype=torch.bool, device=DEV),
            "one": m == (M * 3) // 4}[kind]


def _with_garbage(a, mask):
    """A with its masked rows replaced by finite integer garbage (alternating sign per row)"""
    if mask is None:
        return a
    sign = 1.0 - 2.0 * (torch.arange(a.shape[0], device=DEV) % 2).float()
    return torch.where(mask[:, None], a, (GARBAGE * sign)[:, None].expand_as(a))


# --------------------------------------------------------------------------------------------- the matrix
ENTRIES = {          # name -> (C entry, operand dtype, masked)
    "f32": ("ispk_gemm_tn_f32", torch.float32, False),
    "f32_mask": ("ispk_gemm_tn_f32", torch.float32, True),
    "bf16": ("ispk_gemm_tn_bf16", torch.float32, False),
    "bf16_mask": ("ispk_gemm_tn_bf16", torch.float32, True),
    "b16": ("ispk_gemm_tn_b16", torch.bfloat16, False),         # LDS-DMA when N1, N2 % 8 == 0, else the register kernel
    "b16_mask": ("ispk_gemm_tn_b16", torch.bfloat16, True),     # register kernel
}


def _kernel(entry, N1, N2):
    fn, dt, masked = ENTRIES[entry]
    if dt == torch.float32:
        return BF16 if fn == "ispk_gemm_tn_bf16" else F32
    return DMA if not masked and N1 % 8 == 0 and N2 % 8 == 0 else B16


SHAPES = [    # (M, N1, N2): short ranges and their chunk counts, the XCD mapping's branches, column edges
    (1, 80, 384), (31, 384, 384), (32, 128, 128), (33, 64, 96), (64, 512, 384), (65, 80, 384), (96, 384, 1536),
    (97, 256, 136), (130, 1536, 384), (280, 1536, 1536), (288, 1536, 1536), (4099, 384, 384), (4099, 384, 1536),
    (1000, 80, 384),
    # column edges: N % 8 == 4 (the register kernel's straddling half chunk), DMA zero fill past N1 / N2, both past 128
    (300, 4, 12), (517, 84, 132), (517, 132, 84), (200, 12, 4), (700, 132, 260),
    (300, 8, 136), (517, 264, 8), (700, 136, 264),
]
BENCH_SHAPES = [(32768, 512, 384), (32768, 384, 384), (32768, 1536, 384), (32768, 384, 1536), (32768, 80, 384)]
LAYOUTS = ("a", "b", "c", "d", "e", "f", "g")


def _workspace():
    return runtime.workspace(DEV, 0)


def _window_cols(N2, dt):
    """ldb < N2 for layout (e): B row m = `taps` consecutive rows of a [M + taps - 1, Cc] buffer (aligner.py _windows)"""
    quantum = 8 if dt == torch.bfloat16 else 4
    for taps in (5, 4, 3, 2):
        if N2 % taps == 0 and (N2 // taps) % quantum == 0:
            return N2 // taps
    return None


@functools.lru_cache(maxsize=4)
def _int_operands(M, N1, N2):
    return _ints((M, N1), 1000 + M + 7 * N1), _ints((M + 8, N2), 2000 + M + 11 * N2)


def _operands(M, N1, N2, dt, lay, masked_a):
    """Device A / B buffers of one layout holding the integer operands -> (A Buf, B ptr, ldb, B values [M, N2])."""
    a, b_rows = _int_operands(M, N1, N2)
    q = 8 if dt == torch.bfloat16 else 4          # b16 rows: lda, ldb multiples of 8 (a slice of wider rows for N % 8 == 4)
    wide = lay == "b"
    lda = -(-N1 // q) * q + (2 * q if wide else 0)
    A = Buf(dt, M, N1, lda, 8 if wide else 0)
    A.view.copy_(masked_a.to(dt))
    if lay == "e":
        Cc = _window_cols(N2, dt)
        taps = N2 // Cc
        flat = b_rows.reshape(-1)[: (M + taps - 1) * Cc]
        Bb = Buf(dt, M + taps - 1, Cc, Cc)
        Bb.view.copy_(flat.reshape(M + taps - 1, Cc).to(dt))
        bview = torch.as_strided(Bb.flat, (M, N2), (Cc, 1), 0)
        return A, Bb, Cc, bview.float()
    ldb = -(-N2 // q) * q + (2 * q if wide else 0)
    Bb = Buf(dt, M, N2, ldb, 8 if wide else 0)
    Bb.view.copy_(b_rows[:M].to(dt))
    return A, Bb, ldb, b_rows[:M]


def _c_layout(lay, N1, N2):
    """-> (ldc, offset, accumulate)"""
    return {"a": (N2, 0, False), "b": (N2, 0, False), "c": (N2, 1, False), "d": (N2 + 3, 0, False), "e": (N2, 0, False),
            "f": (N2, 0, True), "g": (N2 + 9, 5, True)}[lay]


def _run_case(entry, M, N1, N2, lay, mask_kind, hits, ws=None):
    """One matrix case; returns a list of failure strings (empty: passed)."""
    fn_name, dt, _ = ENTRIES[entry]
    fn = getattr(runtime.lib(), fn_name)
    what = f"{entry} {M}x{N1}x{N2} layout {lay} mask {mask_kind}"
    mask = _mask(mask_kind, M)
    a_vals, _ = _int_operands(M, N1, N2)
    A, Bb, ldb, b = _operands(M, N1, N2, dt, lay, _with_garbage(a_vals, mask))
    ldc, off, acc = _c_layout(lay, N1, N2)
    C = Buf(torch.float32, N1, N2, ldc, off)
    c0 = _ints((N1, N2), 3000 + N1 + N2, -1024, 1024) if acc else None
    ws = _workspace() if ws is None else ws
    am = a_vals if mask is None else a_vals * mask[:, None].float()
    ref = am.double().T @ b.double()
    if acc:
        ref = ref + c0.double()
    fails, outs = [], []
    bptr = Bb.ptr() if lay != "e" else Bb.flat.data_ptr()
    for _ in range(2):
        C.reset()
        if acc:
            C.view.copy_(c0)
        rc = fn(A.ptr(), A.ld, bptr, ldb, C.ptr(), ldc, M, N1, N2, runtime._ptr(mask), int(acc), ws.data_ptr(),
                ws.numel(), None)
        torch.cuda.synchronize()
        if rc != 0:
            return [f"{what}: rc={rc} {_err()}"]
        outs.append(C.ints.clone())
    kernel, splits, rows_per = _last_plan()
    want_k = _kernel(entry, N1, N2)
    want = _plan(M, N1, N2, 1, want_k == DMA, ws.numel())
    if (kernel, splits, rows_per) != (want_k, *want):
        fails.append(f"{what}: ran kernel {kernel} with plan {splits} x {rows_per}, the mirror says {want_k} with {want}")
    hits.update(_branches(M, N1, N2, 1, kernel, splits, rows_per))
    got = C.view.double()
    if not torch.equal(got, ref):
        bad = (got != ref)
        r, c = [int(v) for v in bad.nonzero()[0]]
        fails.append(f"{what}: {int(bad.sum())} of {N1 * N2} entries differ from the exact sum, first at [{r}, {c}]: "
                     f"{got[r, c].item()} != {ref[r, c].item()}")
    if n := C.outside_touched():
        fails.append(f"{what}: {n} elements outside C's view were written")
    if not torch.equal(outs[0], outs[1]):
        fails.append(f"{what}: a second call wrote different bits")
    return fails


def _matrix():
    cases = []
    for M, N1, N2 in SHAPES + BENCH_SHAPES:
        for entry, (_, dt, masked) in ENTRIES.items():
            masks = ("ragged",) if masked else (None,)
            for lay in LAYOUTS:
                if lay == "e" and _window_cols(N2, dt) is None:
                    continue
                if M == 32768 and lay in ("c", "e"):       # the bench shapes: (a), (b), (d), (f), (g)
                    continue
                for mk in masks:
                    cases.append((entry, M, N1, N2, lay, mk))
            if masked and M != 32768:        # all-false and single-row masks on the contiguous layout (and accumulate)
                for mk in ("none", "one"):
                    cases.append((entry, M, N1, N2, "a", mk))
                    cases.append((entry, M, N1, N2, "f", mk))
    return cases


MATRIX = _matrix()
HITS: set = set()


def _shape_id(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", SHAPES + BENCH_SHAPES, ids=_shape_id)
def test_weight_gradient_matrix_is_exact_on_integers(shape):
    """Every entry x layout x mask case of one shape equals the float64 sum bit for bit, with the plan the mirror predicts,
    no stray stores and identical bits on a second call."""
    fails, n = [], 0
    for case in MATRIX:
        if case[1:4] != shape:
            continue
        n += 1
        fails += _run_case(case[0], *case[1:], hits=HITS)
    print(f"{_shape_id(shape)}: {n} cases, {len(fails)} failed")
    for f in fails:
        print("FAIL", f)
    assert not fails, fails[0]


REQUIRED_BRANCHES = {"k1", "k2", "k3", "k4", "nz<8", "nz%8==0", "nz%8!=0", "splits==1", "chunks=1", "chunks=2", "chunks=3",
                     "short-last", "last-chunks=1", "last-chunks=2", "last-chunks=3"}


def _predicted_hits():
    """branches the matrix reaches by the mirror alone, per kernel"""
    per = {}
    ws = 48 << 20
    for entry, M, N1, N2, lay, mk in MATRIX:
        k = _kernel(entry, N1, N2)
        s, r = _plan(M, N1, N2, 1, k == DMA, ws)
        per.setdefault(k, set()).update(_branches(M, N1, N2, 1, k, s, r))
    return per


def test_planner_branches_are_all_reached():
    """By the mirror (cross-checked against ispk_gemm_tn_last_plan in every matrix case): every plan branch is reached, the
    XCD mapping's three branches (nz % 8 == 0, a remainder with nz > 8, nz < 8) on each 1-D-grid kernel, and the DMA
    kernel's ranges of 1, 2 and 3 chunks (its s_waitcnt vmcnt(0 / 4 / 8) choice)."""
    assert runtime._TN_WORKSPACE_FLOATS == 48 << 20 and _workspace().numel() >= 48 << 20
    per = _predicted_hits()
    everything = set().union(*per.values())
    assert REQUIRED_BRANCHES <= everything, REQUIRED_BRANCHES - everything
    for k in (BF16, B16, DMA):
        assert {"nz<8", "nz%8==0", "nz%8!=0"} <= per[k], (k, per[k])
    assert {"chunks=1", "chunks=2", "chunks=3", "last-chunks=1", "last-chunks=2", "last-chunks=3"} <= per[DMA], per[DMA]
    counts = {}
    for entry, M, N1, N2, lay, mk in MATRIX:
        k = _kernel(entry, N1, N2)
        counts[k] = counts.get(k, 0) + 1
    print(f"{len(MATRIX)} matrix cases; per kernel {dict(sorted(counts.items()))}; branches per kernel "
          f"{ {k: sorted(v) for k, v in sorted(per.items())} }")
    if HITS:        # the matrix ran in this session: what the library reported must cover the same branches
        assert everything <= HITS, everything - HITS


# --------------------------------------------------------------------------------------------- rounding
ROUNDING = [("f32", 4099, 384, 1536), ("f32", 517, 84, 132), ("bf16", 4099, 384, 1536), ("bf16", 517, 132, 84),
            ("b16_mask", 4099, 384, 1536), ("b16", 517, 84, 132), ("b16", 32768, 1536, 384), ("b16", 1000, 80, 384),
            ("bf16", 32768, 384, 384), ("f32", 32768, 80, 384)]


def _b16_rows(t):
    """t rounded to bf16, as a column slice of NaN-padded rows whose stride is a multiple of 8 (what ispk_gemm_tn_b16 needs)"""
    n = t.shape[1]
    wide = torch.full((t.shape[0], -(-n // 8) * 8 + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:, :n] = t.bfloat16()
    return wide[:, :n]


def _normal(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV)


@pytest.mark.parametrize("entry,M,N1,N2", ROUNDING)
def test_weight_gradient_rounding_on_normal_operands(entry, M, N1, N2):
    """fp32: max |C - ref| <= 2e-6 max |ref| against float64 on the fp32 operands; bf16 paths: <= 2e-5 max |ref| against
    float64 on the RNE-rounded operands (no bit-equality between the DMA and register kernels: their range counts, and so
    their summation orders, differ)."""
    fn_name, dt, masked = ENTRIES[entry]
    a, b = _normal((M, N1), 11 + M), _normal((M, N2), 12 + M)
    mask = _mask("ragged", M) if masked else None
    fp32 = fn_name == "ispk_gemm_tn_f32"
    ar = a if fp32 else a.bfloat16().float()
    br = b if fp32 else b.bfloat16().float()
    ref = (ar if mask is None else ar * mask[:, None].float()).double().T @ br.double()
    if dt == torch.bfloat16:
        a, b = _b16_rows(a), _b16_rows(b)
    out = runtime.gemm_tn(a, b, row_mask=mask, bf16=fn_name == "ispk_gemm_tn_bf16")
    assert _last_plan()[0] == _kernel(entry, N1, N2)
    err = (out.double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"{entry} {M}x{N1}x{N2} kernel {_kernel(entry, N1, N2)}: max |C - ref| / max |ref| = {err:.3e}")
    assert err <= (2e-6 if fp32 else 2e-5)


@pytest.mark.parametrize("N1,N2", [(384, 1536), (84, 132), (1536, 384)])
def test_single_row_is_one_exact_outer_product(N1, N2):
    """M = 1: C = a^T b.  Products of bf16 values are exact in fp32, so the bf16-in-flight and bf16-operand paths equal the
    outer product of the RNE-rounded operands bit for bit; the fp32 path is within 1 ulp of the float64 product."""
    a, b = _normal((1, N1), 21 + N1), _normal((1, N2), 22 + N2)
    want = a.bfloat16().float().T @ b.bfloat16().float()        # one product per entry: exact in fp32
    assert torch.equal(runtime.gemm_tn(a, b, bf16=True), want)
    a16, b16 = _b16_rows(a), _b16_rows(b)
    assert torch.equal(runtime.gemm_tn(a16, b16), want)
    assert _last_plan()[0] == (DMA if N1 % 8 == 0 and N2 % 8 == 0 else B16)
    assert torch.equal(runtime.gemm_tn(a16, b16, row_mask=torch.ones(1, dtype=torch.bool, device=DEV)), want)
    assert _last_plan()[0] == B16
    got = runtime.gemm_tn(a, b)
    ref = (a.double().T @ b.double())
    ulp = torch.nextafter(ref.float().abs(), torch.tensor(float("inf"), device=DEV)) - ref.float().abs()
    assert bool(((got.double() - ref).abs() <= ulp.double()).all())


# --------------------------------------------------------------------------------------------- workspace, refusals
def _c_untouched(C):
    return C.outside_touched(torch.zeros(C.n, dtype=torch.bool, device=DEV)) == 0


@pytest.mark.parametrize("entry", ["f32_mask", "bf16", "b16", "b16_mask"])
def test_small_workspaces_cap_the_plan_or_refuse(entry):
    """workspace_floats == N1 N2: one range over all of M; 3 N1 N2: a capped plan of 3 ranges; fewer than N1 N2 floats:
    -3 with a message and C's bits untouched."""
    M, N1, N2 = 32768, 384, 384
    fails, hits = [], set()
    for mult, want_splits in ((1, 1), (3, 3)):
        ws = torch.full((mult * N1 * N2 + SLACK,), float("nan"), device=DEV)[: mult * N1 * N2]
        fails += _run_case(entry, M, N1, N2, "a", "ragged" if ENTRIES[entry][2] else None, hits, ws=ws)
        assert _last_plan()[1] == want_splits
    assert not fails, fails
    fn_name, dt, _ = ENTRIES[entry]
    A, B = Buf(dt, M, N1, N1), Buf(dt, M, N2, N2)
    A.view.zero_()
    B.view.zero_()
    C = Buf(torch.float32, N1, N2, N2)
    ws = torch.empty(N1 * N2, device=DEV)
    rc = getattr(runtime.lib(), fn_name)(A.ptr(), N1, B.ptr(), N2, C.ptr(), N2, M, N1, N2, None, 0, ws.data_ptr(),
                                         N1 * N2 - 1, None)
    torch.cuda.synchronize()
    assert rc == -3 and "workspace" in _err()
    assert _c_untouched(C)


def test_weight_gradient_refusals_leave_c_untouched():
    """Each documented refusal comes back as a non-zero code with a message and writes nothing."""
    lib = runtime.lib()
    M = 64
    A32, B32 = Buf(torch.float32, M, 256, 256, extra=64), Buf(torch.float32, M, 256, 256)
    A16, B16b = Buf(torch.bfloat16, M, 256, 256, extra=64), Buf(torch.bfloat16, M, 256, 256)
    for t in (A32, B32, A16, B16b):
        t.flat.zero_()
    C = Buf(torch.float32, 256, 256, 256)
    ws = _workspace()
    w = (ws.data_ptr(), ws.numel(), None)
    f32, b16 = lib.ispk_gemm_tn_f32, lib.ispk_gemm_tn_b16
    a32 = A32.flat.data_ptr()
    cases = [
        ("N1 % 4 != 0", lambda: f32(a32, 256, B32.ptr(), 256, C.ptr(), 256, M, 6, 64, None, 0, *w)),
        ("lda % 4 != 0", lambda: f32(a32, 130, B32.ptr(), 256, C.ptr(), 256, M, 64, 64, None, 0, *w)),
        ("A not 16-byte aligned", lambda: f32(a32 + 4, 256, B32.ptr(), 256, C.ptr(), 256, M, 64, 64, None, 0, *w)),
        ("b16 lda % 8 != 0", lambda: b16(A16.flat.data_ptr(), 132, B16b.ptr(), 256, C.ptr(), 256, M, 128, 64, None, 0, *w)),
        ("M = 0", lambda: f32(a32, 256, B32.ptr(), 256, C.ptr(), 256, 0, 64, 64, None, 0, *w)),
        ("ldc < N2", lambda: f32(a32, 256, B32.ptr(), 256, C.ptr(), 60, M, 64, 64, None, 0, *w)),
        ("splits * batch > 65535", lambda: lib.ispk_gemm_tn_batched_f32(a32, 4, 0, B32.ptr(), 4, 0, C.ptr(), 4, 0, 70000, 1,
                                                                         4, 4, None, 0, *w)),
    ]
    for what, call in cases:
        rc = call()
        torch.cuda.synchronize()
        assert rc != 0 and _err(), what
        if what == "splits * batch > 65535":
            assert rc == -4, (what, rc)
        assert _c_untouched(C), f"{what}: refused call wrote C"


# --------------------------------------------------------------------------------------------- batched
@pytest.mark.parametrize("batch,M,N1,N2", [(1, 130, 64, 64), (3, 130, 64, 64), (8, 130, 64, 64), (5, 97, 132, 264),
                                           (2, 700, 256, 128), (9, 33, 20, 36)])
def test_batched_weight_gradients_with_padded_strides_and_masks(batch, M, N1, N2):
    """ispk_gemm_tn_batched_f32 with padded stride_a / stride_b / stride_c, ldc > N2 and C at an offset (aligner.py's
    out=dq_buf[:, :n]), with and without the [batch][M] row mask, plain and accumulating: integer-exact per item, nothing
    written between or around the items, plan as mirrored.  batch x splits falls on both sides of multiples of 8."""
    lib = runtime.lib()
    lda, ldb, ldc = N1 + 12, N2 + 8, N2 + 7
    sa, sb, sc = M * lda + 16, M * ldb + 4, N1 * ldc + 5
    a = _ints((batch, M, N1), 41 + batch + M)
    b = _ints((batch, M, N2), 42 + batch + M)
    mask = (torch.arange(batch * M, device=DEV).reshape(batch, M) % 3 != (torch.arange(batch, device=DEV) % 3)[:, None])
    Abuf = torch.full((batch * sa + SLACK,), float("nan"), device=DEV)
    Bbuf = torch.full((batch * sb + SLACK,), float("nan"), device=DEV)
    av = torch.as_strided(Abuf, (batch, M, N1), (sa, lda, 1))
    bv = torch.as_strided(Bbuf, (batch, M, N2), (sb, ldb, 1))
    bv.copy_(b)
    C = Buf(torch.float32, 1, batch * sc + 3, batch * sc + 3)
    cview = torch.as_strided(C.flat, (batch, N1, N2), (sc, ldc, 1), 3)
    inside = torch.zeros(C.n, dtype=torch.bool, device=DEV)
    torch.as_strided(inside, (batch, N1, N2), (sc, ldc, 1), 3).fill_(True)
    c0 = _ints((batch, N1, N2), 43, -1024, 1024)
    ws = _workspace()
    for masked in (False, True):
        for acc in (False, True):
            av.copy_(torch.where(mask[..., None], a, GARBAGE) if masked else a)
            am = a * mask[..., None].float() if masked else a
            ref = am.double().transpose(1, 2) @ b.double() + (c0.double() if acc else 0)
            outs = []
            for _ in range(2):
                C.reset()
                if acc:
                    cview.copy_(c0)
                rc = lib.ispk_gemm_tn_batched_f32(Abuf.data_ptr(), lda, sa, Bbuf.data_ptr(), ldb, sb, C.ptr() + 12, ldc, sc,
                                                  batch, M, N1, N2, mask.data_ptr() if masked else None,
                                                  int(acc), ws.data_ptr(), ws.numel(), None)
                torch.cuda.synchronize()
                assert rc == 0, _err()
                outs.append(C.ints.clone())
            what = f"masked={masked} accumulate={acc}"
            k, splits, rows_per = _last_plan()
            assert (k, splits, rows_per) == (F32, *_plan(M, N1, N2, batch, False, ws.numel())), what
            assert torch.equal(cview.double(), ref), what
            assert C.outside_touched(inside) == 0, what
            assert torch.equal(outs[0], outs[1]), what
    # the runtime wrapper on the same strided views (it passes no mask)
    C.reset()
    av.copy_(a)
    runtime.gemm_tn_batched(av, bv, out=cview)
    assert torch.equal(cview.double(), a.double().transpose(1, 2) @ b.double())
    assert C.outside_touched(inside) == 0


# --------------------------------------------------------------------------------------------- zero rows
def test_zero_rows_give_zero_gradients():
    """A sum over no rows is zero: gemm_tn / gemm_tn_batched / colsum / smallk_wgrad return zeros (strided `out` views
    included, nothing around them written), leave `out` untouched under accumulate, and never reach the C entries, which
    keep refusing M = 0."""
    for dt in (torch.float32, torch.bfloat16):
        for bf16 in (False, True) if dt == torch.float32 else (False,):
            z = runtime.gemm_tn(torch.empty(0, 80, dtype=dt, device=DEV), torch.empty(0, 384, dtype=dt, device=DEV), bf16=bf16)
            assert z.shape == (80, 384) and not bool(z.any())
            C = Buf(torch.float32, 80, 384, 400, 3)
            runtime.gemm_tn(torch.empty(0, 80, dtype=dt, device=DEV), torch.empty(0, 384, dtype=dt, device=DEV), out=C.view,
                            bf16=bf16, row_mask=torch.empty(0, dtype=torch.bool, device=DEV))
            assert not bool(C.view.any()) and C.outside_touched() == 0
            before = C.ints.clone()
            runtime.gemm_tn(torch.empty(0, 80, dtype=dt, device=DEV), torch.empty(0, 384, dtype=dt, device=DEV), out=C.view,
                            accumulate=True, bf16=bf16)
            assert torch.equal(C.ints, before)
    C = Buf(torch.float32, 1, 3 * 1000, 3 * 1000)
    cview = torch.as_strided(C.flat, (3, 20, 36), (1000, 40, 1), 2)
    runtime.gemm_tn_batched(torch.empty(3, 0, 20, device=DEV), torch.empty(3, 0, 36, device=DEV), out=cview)
    inside = torch.zeros(C.n, dtype=torch.bool, device=DEV)
    torch.as_strided(inside, (3, 20, 36), (1000, 40, 1), 2).fill_(True)
    assert not bool(cview.any()) and C.outside_touched(inside) == 0
    s = runtime.colsum(torch.empty(0, 384, device=DEV), row_mask=torch.empty(0, dtype=torch.bool, device=DEV))
    assert s.shape == (384,) and not bool(s.any())
    w = runtime.smallk_wgrad(torch.empty(0, 256, device=DEV), torch.empty(0, 2, device=DEV))
    assert w.shape == (256, 2) and not bool(w.any())
    # the C entries keep their documented M >= 1 / rows >= 1 refusal
    lib, one = runtime.lib(), torch.zeros(64, device=DEV)
    ws = _workspace()
    p = one.data_ptr()
    assert lib.ispk_gemm_tn_f32(p, 4, p, 4, p, 4, 0, 4, 4, None, 0, ws.data_ptr(), ws.numel(), None) != 0
    assert lib.ispk_colsum_f32(p, 4, 0, 4, None, ws.data_ptr(), ws.numel(), p, None) != 0
    assert lib.ispk_smallk_wgrad_f32(p, 4, p, 4, 0, 4, 2, ws.data_ptr(), ws.numel(), p, None) != 0


# --------------------------------------------------------------------------------------------- colsum, small-K
COLSUM_ROWS = (1, 255, 256, 257, 9001, 32768)


@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_colsum_is_exact_on_integers(rows):
    """ispk_colsum_f32 over rows below, at and past its 256 partial blocks, cols up to 1536, contiguous and strided
    (ldx > cols), with no mask, a ragged mask and an all-false mask (masked rows hold +-2^20 garbage): bit-exact, nothing
    written past `out`, and the workspace refusal."""
    lib, ws = runtime.lib(), _workspace()
    fails = []
    for cols in (1, 80, 384, 1536):
        x = _ints((rows, cols), 51 + rows + cols)
        for ldx in (cols, cols + 5):
            X = Buf(torch.float32, rows, cols, ldx)
            for mk in (None, "ragged", "none"):
                mask = _mask(mk, rows)
                X.reset()
                X.view.copy_(_with_garbage(x, mask))
                ref = (x if mask is None else x * mask[:, None].float()).double().sum(0)
                out = Buf(torch.float32, 1, cols, cols)
                rc = lib.ispk_colsum_f32(X.ptr(), ldx, rows, cols, runtime._ptr(mask), ws.data_ptr(), ws.numel(), out.ptr(),
                                         None)
                torch.cuda.synchronize()
                what = f"colsum rows={rows} cols={cols} ldx={ldx} mask={mk}"
                if rc != 0:
                    fails.append(f"{what}: rc={rc} {_err()}")
                    continue
                if not torch.equal(out.view[0].double(), ref):
                    fails.append(f"{what}: {int((out.view[0].double() != ref).sum())} sums differ")
                if out.outside_touched():
                    fails.append(f"{what}: wrote past out")
        if rows == 256:
            out = Buf(torch.float32, 1, cols, cols)
            rc = lib.ispk_colsum_f32(X.ptr(), cols, rows, cols, None, ws.data_ptr(), 256 * cols - 1, out.ptr(), None)
            torch.cuda.synchronize()
            assert rc != 0 and "workspace" in _err() and _c_untouched(out)
    assert torch.equal(runtime.colsum(x), x.double().sum(0).float())
    for f in fails:
        print("FAIL", f)
    assert not fails, fails[0]


@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_smallk_wgrad_is_exact_on_integers(rows):
    """ispk_smallk_wgrad_f32 (out[n][k] = sum_r g[r][n] x[r][k]) for K in {1, 2, 3, 8} and N up to 1536, contiguous and
    strided (ldg > N, ldx > K): bit-exact, nothing written past `out`, and the workspace refusal."""
    lib, ws = runtime.lib(), _workspace()
    fails = []
    for N in (1, 80, 384, 1536):
        for K in (1, 2, 3, 8):
            g = _ints((rows, N), 61 + rows + N)
            x = _ints((rows, K), 62 + rows + K)
            ref = g.double().T @ x.double()
            for ldg, ldx in ((N, K), (N + 3, K + 5)):
                G, X = Buf(torch.float32, rows, N, ldg), Buf(torch.float32, rows, K, ldx)
                G.view.copy_(g)
                X.view.copy_(x)
                out = Buf(torch.float32, N, K, K)
                rc = lib.ispk_smallk_wgrad_f32(G.ptr(), ldg, X.ptr(), ldx, rows, N, K, ws.data_ptr(), ws.numel(), out.ptr(),
                                               None)
                torch.cuda.synchronize()
                what = f"smallk rows={rows} N={N} K={K} ldg={ldg} ldx={ldx}"
                if rc != 0:
                    fails.append(f"{what}: rc={rc} {_err()}")
                    continue
                if not torch.equal(out.view.double(), ref):
                    fails.append(f"{what}: {int((out.view.double() != ref).sum())} entries differ")
                if out.outside_touched():
                    fails.append(f"{what}: wrote past out")
            if rows == 256 and N == 80:
                out = Buf(torch.float32, N, K, K)
                rc = lib.ispk_smallk_wgrad_f32(G.ptr(), ldg, X.ptr(), ldx, rows, N, K, ws.data_ptr(), 256 * N * K - 1,
                                               out.ptr(), None)
                torch.cuda.synchronize()
                assert rc != 0 and "workspace" in _err() and _c_untouched(out)
    assert torch.equal(runtime.smallk_wgrad(g, x), ref.float())
    for f in fails:
        print("FAIL", f)
    assert not fails, fails[0]
