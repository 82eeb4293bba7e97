"""Layout / epilogue matrix of the GEMM entry points (ispk_gemm_bf16, its split-K twin, ispk_gemm_f32 and
ispk_gemm_f32_batched) against float64 on the same bf16-rounded operands.

For every bf16 kernel the dispatcher can pick (panel, row-block, split-K, generic tile) a few shapes that reach it are run
through each epilogue the ABI accepts and each operand layout below.  Every case checks:
  * accuracy against float64 (fp32 out: max abs error < 2e-5; bf16 out: |C - ref| <= |ref| 2^-8 + 1e-5), masked entries 0;
  * no stray stores: C lives inside a larger buffer filled with a NaN sentinel, and everything outside C's view
    (padding columns, rows past M, the gap before an offset view, the gap between batches) must keep the sentinel's bits;
  * the kernel that ran, for the aligned layouts (a) and (b), so that a change of the dispatch rules fails here loudly
    instead of silently moving the other tests' coverage to another kernel;
  * determinism: a second call writes the same bits.
Layouts: (a) contiguous; (b) A / C / resid as column slices of wider buffers that keep 16-byte alignment; (c) C one element
past an aligned address; (d) C and resid with a leading dimension of N + 3; (e) bias = full[1:N+1]; (f) W a column slice
(ldw > K).  Input padding is NaN too, so a kernel that reads outside its operands' views shows up as NaN output."""
import functools

import pytest
import torch
import torch.nn.functional as F

from isp_tts_amd import runtime, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLACK = 256                    # elements after every backing buffer: a stray store past the view lands inside it
NAN32 = 0x7FC0_1234            # sentinel bit patterns (quiet NaNs with a payload no kernel produces)
NAN16 = 0x7FC1
LAYOUTS = ("a", "b", "c", "d", "e", "f")

SHAPES = {
    "panel": [(6400, 384, 384), (515, 1024, 256), (1, 64, 256)],
    "rowblock": [(8200, 384, 1536), (33000, 80, 768)],
    "splitk": [(800, 384, 1536), (77, 256, 1024), (1, 384, 1536)],
    "tile": [(300, 320, 768), (300, 3, 264)],
}


# --------------------------------------------------------------------------------------------- operands and reference
@functools.lru_cache(maxsize=2)
def _operands(M, N, K):
    """bf16-rounded A [M, K], W [N, K] (as fp32 values, exact in both dtypes), their float64 product, and epilogue inputs."""
    a = synth._normal(f"t/gl/a{M}x{K}", (M, K)).to(torch.bfloat16).float()
    w = (synth._normal(f"t/gl/w{N}x{K}", (N, K), K ** -0.5)).to(torch.bfloat16).float()
    acc = a.double() @ w.double().T
    return dict(a=a, w=w, acc=acc, bias=synth._normal(f"t/gl/b{N}", (N,)), bias_m=synth._normal(f"t/gl/bm{M}", (M,)),
                resid=synth._normal(f"t/gl/r{M}x{N}", (M, N)), mask=torch.arange(M) % 5 != 2,
                mask_n=torch.arange(N) % 3 != 1)


def _ref(o, e):
    v = o["acc"]
    if e.get("bias"):
        v = v + (o["bias_m"].double()[:, None] if e.get("bias_row") else o["bias"].double())
    if e.get("act") == "gelu":
        v = F.gelu(v)
    if e.get("act") == "silu":
        v = F.silu(v)
    mk = None
    if e.get("mask"):
        mk = (o["mask_n"][None, :] if e.get("mask_col") else o["mask"][:, None]).double()
    if e["mask"] == "acc":
        v = v * mk
    if e.get("resid"):
        r = o["resid"].to(torch.bfloat16) if e["resid"] == "bf16" else o["resid"]
        v = v + r.double()
    if e["mask"] == "out":
        v = v * mk
    return v, mk


# Epilogues of the ispk_gemm_bf16 entry (runtime.gemm).  out: C dtype; resid: fp32 / bf16; mask: row mask applied before
# ("acc") or after ("out") the residual, per column with mask_col.
EPILOGUES_BF16 = {
    "none": dict(out="f32"),
    "bias": dict(out="f32", bias=True),
    "bias_gelu": dict(out="f32", bias=True, act="gelu"),
    "silu": dict(out="f32", act="silu"),
    "resid_f32": dict(out="f32", resid="f32"),
    "resid_bf16": dict(out="f32", resid="bf16"),
    "mask_acc": dict(out="f32", bias=True, resid="f32", mask="acc"),
    "mask_out": dict(out="f32", resid="bf16", mask="out"),
    "out_bf16": dict(out="bf16"),
    "out_bf16_bias_gelu": dict(out="bf16", bias=True, act="gelu"),
    "out_bf16_mask_out": dict(out="bf16", bias=True, mask="out"),
    "out_bf16_resid_bf16": dict(out="bf16", resid="bf16", mask="acc"),
    "bias_row": dict(out="f32", bias=True, bias_row=True, act="silu"),
    "mask_col": dict(out="f32", resid="f32", mask="out", mask_col=True),
    "out_bf16_mask_col": dict(out="bf16", bias=True, mask="acc", mask_col=True),
}
EPILOGUES_F32 = {k: v for k, v in EPILOGUES_BF16.items() if v["out"] == "f32" and v.get("resid") != "bf16"}

for _e in list(EPILOGUES_BF16.values()):
    _e.setdefault("mask", None)


def _flags(e):
    f = 0
    f |= runtime.EP_GELU if e.get("act") == "gelu" else 0
    f |= runtime.EP_SILU if e.get("act") == "silu" else 0
    f |= {"acc": runtime.EP_MASK_ACC, "out": runtime.EP_MASK_OUT, None: 0}[e["mask"]]
    f |= runtime.EP_BIAS_ROW if e.get("bias_row") else 0
    f |= runtime.EP_MASK_COL if e.get("mask_col") else 0
    return f


# --------------------------------------------------------------------------------------------- buffers
class Buf:
    """A flat device buffer filled with the sentinel and one strided 2-D view [rows, cols] of it."""

    def __init__(self, dtype, rows, cols, ld, off, fill=None):
        self.dtype, self.rows, self.cols, self.ld, self.off = dtype, rows, cols, ld, off
        self.n = off + max(rows, 1) * ld + SLACK
        self.idx = (off + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]).reshape(-1)
        self.flat = torch.empty(self.n, dtype=dtype, device=DEV)
        self.reset()
        if fill is not None:
            self.view.copy_(fill.to(dtype).to(DEV))

    def reset(self):
        ints = torch.int16 if self.dtype == torch.bfloat16 else torch.int32
        self.flat.view(ints).fill_(NAN16 if self.dtype == torch.bfloat16 else NAN32)

    @property
    def view(self):
        return torch.as_strided(self.flat, (self.rows, self.cols), (self.ld, 1), self.off)

    def bits(self):
        return self.flat.view(torch.int16 if self.dtype == torch.bfloat16 else torch.int32).cpu()

    def outside_touched(self, idx=None):
        """number of elements outside the view (or outside the given element index set) whose bits changed"""
        sentinel = NAN16 if self.dtype == torch.bfloat16 else NAN32
        keep = torch.ones(self.n, dtype=torch.bool)
        keep[self.idx if idx is None else idx] = False
        return int((self.bits()[keep] != sentinel).sum())


def _layout(lay, o, e, M, N, K, dt, inputs):
    """Device operands of one case: A, W (bf16 or fp32 per dt), C buffer, resid, bias, mask.  `inputs` caches the A / W
    buffers of a shape (the kernels only read them)."""
    a_ld, a_off = (K + 64, 32) if lay == "b" else (K, 0)
    w_ld = K + 8 if lay == "f" else K
    c_ld, c_off = {"b": (N + 16, 8), "c": (N, 1), "d": (N + 3, 0)}.get(lay, (N, 0))
    out_dt = torch.bfloat16 if e["out"] == "bf16" else torch.float32
    if ("A", a_ld) not in inputs:
        inputs[("A", a_ld)] = Buf(dt, M, K, a_ld, a_off, o["a"])
    if ("W", w_ld) not in inputs:
        inputs[("W", w_ld)] = Buf(dt, N, K, w_ld, 0, o["w"])
    A, W = inputs[("A", a_ld)], inputs[("W", w_ld)]
    C = Buf(out_dt, M, N, c_ld, c_off)
    R = None
    if e.get("resid"):
        r_dt = torch.bfloat16 if e["resid"] == "bf16" else torch.float32
        r_ld, r_off = {"b": (N + 16, 8), "d": (N + 3, 0)}.get(lay, (N, 0))
        R = Buf(r_dt, M, N, r_ld, r_off, o["resid"])
    bias = None
    if e.get("bias"):
        bv = o["bias_m"] if e.get("bias_row") else o["bias"]
        full = torch.full((bv.numel() + 8,), float("nan"), device=DEV)
        bias = full[1:bv.numel() + 1] if lay == "e" else full[:bv.numel()]
        bias.copy_(bv.to(DEV))
    mask = None
    if e["mask"]:
        mask = (o["mask_n"] if e.get("mask_col") else o["mask"]).to(DEV)
    return A, W, C, R, bias, mask


def _check_values(C, ref, mk, e, what, fails):
    got = C.view.cpu().double()
    if C.dtype == torch.bfloat16:
        bad = ~((got - ref).abs() <= ref.abs() * 2 ** -8 + 1e-5)
        if bad.any():
            fails.append(f"{what}: {int(bad.sum())} bf16 outputs off (max err {(got - ref).abs().max().item():.3g})")
    else:
        err = (got - ref).abs().max().item() if got.numel() else 0.0
        if not err < 2e-5:
            fails.append(f"{what}: max |C - ref| = {err:.3g}")
    if e["mask"] == "out" and mk is not None and got.numel():
        masked = (mk.expand_as(got) == 0)
        if masked.any() and not (got[masked] == 0).all():
            fails.append(f"{what}: masked outputs are not 0")
    n = C.outside_touched()
    if n:
        fails.append(f"{what}: {n} elements outside C's view were written")


def _kernel_of(label):
    """profiler label of a runtime.gemm launch -> the dispatch path"""
    for key, path in (("gemm_bf16_splitk", "splitk"), ("gemm_bf16_panel", "panel"), ("gemm_bf16_wide", "rowblock"),
                      ("gemm_bf16_kernel", "tile"), ("gemm_f32_kernel", "f32")):
        if label.startswith(key):
            return path
    return label


def _expected_bf16_path(path, e):
    """The kernel the dispatcher must choose for an aligned layout: the fast paths do not serve per-row bias, per-column
    masks, bf16 C with a residual (panel) or bf16 C at all (row-block); those go to the generic tile kernel."""
    if e.get("bias_row") or e.get("mask_col"):
        return "tile"
    if path == "panel" and e["out"] == "bf16" and e.get("resid"):
        return "tile"
    if path == "rowblock" and e["out"] == "bf16":
        return "tile"
    return path


def _variant_range(path):
    return {"panel": 1, "rowblock": 2, "splitk": 2, "tile": 3}[path]


def _gemm_call(A, W, C, R, bias, mask, flags):
    prof = runtime.LaunchProfiler()
    runtime.set_profiler(prof)
    try:
        runtime.gemm(A.view, W.view, bias=bias, resid=None if R is None else R.view, mask=mask, flags=flags, out=C.view)
    finally:
        runtime.set_profiler(None)
    torch.cuda.synchronize()
    return prof.records[-1][0] if prof.records else None


def _run_matrix(path, M, N, K, dt, epilogues):
    lib = runtime.lib()
    o = _operands(M, N, K)
    fails, ncases, inputs = [], 0, {}
    for ename, e in epilogues.items():
        ref, mk = _ref(o, e)
        for lay in LAYOUTS:
            if lay == "e" and not e.get("bias"):
                continue
            what = f"{path} {M}x{N}x{K} {'bf16' if dt == torch.bfloat16 else 'f32'} x {ename} x layout {lay}"
            ncases += 1
            A, W, C, R, bias, mask = _layout(lay, o, e, M, N, K, dt, inputs)
            flags = _flags(e)
            try:
                label = _gemm_call(A, W, C, R, bias, mask, flags)
            except runtime.IspkError as ex:
                fails.append(f"{what}: refused: {ex}")
                continue
            _check_values(C, ref, mk, e, what, fails)
            kernel = _kernel_of(label)
            if dt == torch.bfloat16:
                if lay in ("a", "b"):
                    want = _expected_bf16_path(path, e)
                    v = lib.ispk_gemm_bf16_last_variant()
                    if kernel != want or (M > 0 and v // 1000 != _variant_range(want)):
                        fails.append(f"{what}: ran {label} (variant {v}), expected the {want} kernel")
                # the runtime's split-K guard mirrors the entry's own check: where the plan splits but the runtime did
                # not, the split-K entry must refuse these very arguments
                full_flags = flags | (runtime.EP_OUT_BF16 if e["out"] == "bf16" else 0) | \
                    (runtime.EP_RESID_BF16 if e.get("resid") == "bf16" else 0)
                ks = lib.ispk_gemm_bf16_splitk_plan(M, N, K, full_flags) if M < 2048 and K >= 512 else 1
                if ks > 1 and kernel != "splitk":
                    ws = torch.empty(ks * M * N, device=DEV)
                    before = C.bits()
                    rc = lib.ispk_gemm_bf16_splitk(A.view.data_ptr(), A.ld, W.view.data_ptr(), W.ld, C.view.data_ptr(), C.ld,
                                                   runtime._ptr(bias), None if R is None else R.view.data_ptr(),
                                                   0 if R is None else R.ld, runtime._ptr(mask), M, N, K, full_flags,
                                                   ws.data_ptr(), ks, None)
                    torch.cuda.synchronize()
                    if rc >= 0 or not lib.ispk_last_error_string() or not torch.equal(before, C.bits()):
                        fails.append(f"{what}: runtime skipped split-K (plan {ks}) but ispk_gemm_bf16_splitk accepted (rc={rc})")
            elif kernel != "f32":
                fails.append(f"{what}: ran {label}")
            # determinism: the same call again writes the same bits (split-K included: ordered combine)
            first = C.bits()
            C.reset()
            _gemm_call(A, W, C, R, bias, mask, flags)
            if not torch.equal(first, C.bits()):
                fails.append(f"{what}: second call differs")
    for f in fails:
        print("FAIL", f)
    return fails, ncases


# --------------------------------------------------------------------------------------------- bf16 entry, per path
@pytest.mark.parametrize("path,M,N,K", [(p, *s) for p, shapes in SHAPES.items() for s in shapes])
def test_gemm_bf16_layout_matrix(path, M, N, K):
    lib = runtime.lib()
    # the shape reaches the intended kernel at all (the matrix below then pins it per epilogue and layout)
    plan = lib.ispk_gemm_bf16_splitk_plan(M, N, K, 0)
    assert (plan > 1) == (path == "splitk"), (path, plan)
    fails, n = _run_matrix(path, M, N, K, torch.bfloat16, EPILOGUES_BF16)
    assert n >= 80
    assert not fails, f"{len(fails)} of {n} cases failed, first: {fails[0]}"


# --------------------------------------------------------------------------------------------- fp32 entry, every tile
@pytest.mark.parametrize("M,N,K,tile", [(6400, 384, 384, 12), (515, 1024, 256, 12), (8200, 384, 1536, 12),
                                        (33000, 80, 768, 22), (800, 384, 1536, 12), (300, 3, 264, 11), (1, 64, 256, 11)])
def test_gemm_f32_layout_matrix(M, N, K, tile):
    assert runtime.lib().ispk_gemm_f32_tile(M, N, K) == tile
    fails, n = _run_matrix("f32", M, N, K, torch.float32, EPILOGUES_F32)
    assert not fails, f"{len(fails)} of {n} cases failed, first: {fails[0]}"


# --------------------------------------------------------------------------------------------- batched (transposed) store
@pytest.mark.parametrize("entry,M,N,K", [("bf16", 80, 600, 384), ("bf16", 33, 96, 1024), ("f32", 80, 600, 384),
                                         ("f32", 33, 96, 1024)])
def test_gemm_batched_store(entry, M, N, K):
    """cols_per_batch > 0: C[(j / cpb) * batch_stride + i * ldc + j % cpb] (to_mel: A = weight, W = activations of
    N / cpb utterances).  The gaps between batches, the padding past cpb and the gap before an offset view stay untouched."""
    lib = runtime.lib()
    o = _operands(M, N, K)
    dt = torch.bfloat16 if entry == "bf16" else torch.float32
    fn = lib.ispk_gemm_bf16 if entry == "bf16" else lib.ispk_gemm_f32
    cpb = N // 3
    epis = {
        "plain": dict(out="f32", mask=None),
        "to_mel": dict(out="f32", bias=True, bias_row=True, mask="out", mask_col=True),
        "gelu_mask_acc": dict(out="f32", bias=True, act="gelu", mask="acc"),
    }
    if entry == "bf16":
        epis["out_bf16"] = dict(out="bf16", bias=True, bias_row=True, mask="out", mask_col=True)
    fails = []
    for ename, e in epis.items():
        ref, mk = _ref(o, e)
        for lay, (ldc, gap, off) in {"a": (cpb, 0, 0), "c": (cpb, 0, 1), "d": (cpb + 3, 5, 0)}.items():
            what = f"{entry} batched {M}x{N}x{K} x {ename} x layout {lay}"
            out_dt = torch.bfloat16 if e["out"] == "bf16" else torch.float32
            bstride = M * ldc + gap
            nb = N // cpb
            C = Buf(out_dt, nb * bstride // ldc + 1, ldc, ldc, off)          # flat storage; the index set below is C's
            j = torch.arange(N)
            idx = (off + (j // cpb)[None, :] * bstride + torch.arange(M)[:, None] * ldc + (j % cpb)[None, :])
            A, W = Buf(dt, M, K, K, 0, o["a"]), Buf(dt, N, K, K, 0, o["w"])
            flags = _flags(e) | (runtime.EP_OUT_BF16 if e["out"] == "bf16" else 0)
            bias = None
            if e.get("bias"):
                bias = (o["bias_m"] if e.get("bias_row") else o["bias"]).to(DEV)
            mask = None if not e["mask"] else (o["mask_n"] if e.get("mask_col") else o["mask"]).to(DEV)
            outs = []
            for _ in range(2):
                C.reset()
                rc = fn(A.view.data_ptr(), K, W.view.data_ptr(), K, C.flat.data_ptr() + off * C.flat.element_size(), ldc,
                        runtime._ptr(bias), None, 0, runtime._ptr(mask), M, N, K, flags, cpb, bstride, None)
                torch.cuda.synchronize()
                if rc != 0:
                    fails.append(f"{what}: rc={rc} {lib.ispk_last_error_string()}")
                    break
                outs.append(C.bits())
            if len(outs) < 2:
                continue
            if entry == "bf16" and lib.ispk_gemm_bf16_last_variant() // 1000 != 3:
                fails.append(f"{what}: batched store ran variant {lib.ispk_gemm_bf16_last_variant()}, not the tile kernel")
            got = C.flat.cpu()[idx.reshape(-1)].reshape(M, N).double()
            if out_dt == torch.bfloat16:
                if not ((got - ref).abs() <= ref.abs() * 2 ** -8 + 1e-5).all():
                    fails.append(f"{what}: bf16 outputs off")
            elif not (got - ref).abs().max().item() < 2e-5:
                fails.append(f"{what}: max |C - ref| = {(got - ref).abs().max().item():.3g}")
            if e["mask"] == "out" and not (got[(mk.expand_as(got) == 0)] == 0).all():
                fails.append(f"{what}: masked outputs are not 0")
            if n := C.outside_touched(idx.reshape(-1)):
                fails.append(f"{what}: {n} elements outside the batched view were written")
            if not torch.equal(outs[0], outs[1]):
                fails.append(f"{what}: second call differs")
    for f in fails:
        print("FAIL", f)
    assert not fails, fails[0]


# --------------------------------------------------------------------------------------------- refusals and edges
def _err():
    s = runtime.lib().ispk_last_error_string()
    return s.decode() if s else ""


def test_gemm_documented_refusals_leave_c_untouched():
    """Combinations the ABI refuses come back as a negative code with a message, never as a (wrong) result."""
    lib = runtime.lib()
    M, N, K = 64, 96, 256
    o = _operands(M, N, K)
    A16, W16 = Buf(torch.bfloat16, M, K, K, 0, o["a"]), Buf(torch.bfloat16, N, K, K, 0, o["w"])
    A32, W32 = Buf(torch.float32, M, K, K, 0, o["a"]), Buf(torch.float32, N, K, K, 0, o["w"])
    R = Buf(torch.float32, M, N, N, 0, o["resid"])
    C = Buf(torch.float32, 3 * M, N, N, 0)
    bias = o["bias"].to(DEV)
    cases = [
        ("bf16: resid with a batched store", lib.ispk_gemm_bf16, A16, W16, R.view.data_ptr(), 0, N // 3),
        ("f32: resid with a batched store", lib.ispk_gemm_f32, A32, W32, R.view.data_ptr(), 0, N // 3),
        ("bf16: GELU and SILU together", lib.ispk_gemm_bf16, A16, W16, None, runtime.EP_GELU | runtime.EP_SILU, 0),
        ("f32: GELU and SILU together", lib.ispk_gemm_f32, A32, W32, None, runtime.EP_GELU | runtime.EP_SILU, 0),
        ("f32: bf16 output flag", lib.ispk_gemm_f32, A32, W32, None, runtime.EP_OUT_BF16, 0),
        ("bf16: N % cols_per_batch != 0", lib.ispk_gemm_bf16, A16, W16, None, 0, 7),
        ("bf16: mask flag without a mask", lib.ispk_gemm_bf16, A16, W16, None, runtime.EP_MASK_OUT, 0),
    ]
    for what, fn, A, W, resid, flags, cpb in cases:
        rc = fn(A.view.data_ptr(), K, W.view.data_ptr(), K, C.flat.data_ptr(), N, bias.data_ptr(), resid,
                N if resid else 0, None, M, N, K, flags, cpb, M * N, None)
        torch.cuda.synchronize()
        assert rc < 0 and _err(), what
        assert C.outside_touched(torch.zeros(0, dtype=torch.long)) == 0, f"{what}: refused call wrote C"
    # the split-K entry refuses layouts its plan cannot see (vec_epilogue_ok)
    M, N, K = 800, 384, 1536
    o = _operands(M, N, K)
    ks = lib.ispk_gemm_bf16_splitk_plan(M, N, K, 0)
    assert ks > 1
    A, W = Buf(torch.bfloat16, M, K, K, 0, o["a"]), Buf(torch.bfloat16, N, K, K, 0, o["w"])
    ws = torch.empty(ks * M * N, device=DEV)
    for lay, (ld, off) in {"offset C": (N, 1), "ldc % 4 != 0": (N + 3, 0)}.items():
        C = Buf(torch.float32, M, N, ld, off)
        rc = lib.ispk_gemm_bf16_splitk(A.view.data_ptr(), K, W.view.data_ptr(), K, C.view.data_ptr(), ld, None, None, 0,
                                       None, M, N, K, 0, ws.data_ptr(), ks, None)
        torch.cuda.synchronize()
        assert rc < 0 and _err(), lay
        assert C.outside_touched(torch.zeros(0, dtype=torch.long)) == 0, lay
    full = torch.zeros(N + 1, device=DEV)
    C = Buf(torch.float32, M, N, N, 0)
    assert lib.ispk_gemm_bf16_splitk(A.view.data_ptr(), K, W.view.data_ptr(), K, C.view.data_ptr(), N, full[1:].data_ptr(),
                                     None, 0, None, M, N, K, 0, ws.data_ptr(), ks, None) < 0 and _err()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_gemm_zero_rows(dt):
    """M = 0 launches nothing on any path (split-K shapes included), writes nothing and is not an error."""
    lib = runtime.lib()
    for N, K in ((384, 1536), (384, 384), (80, 768)):
        A, W = Buf(dt, 0, K, K, 0), Buf(dt, N, K, K, 0, torch.ones(N, K))
        C = Buf(torch.float32, 0, N, N, 0)
        out = runtime.gemm(A.view, W.view, out=C.view, flags=runtime.EP_GELU, bias=torch.ones(N, device=DEV))
        torch.cuda.synchronize()
        assert out.shape == (0, N) and C.outside_touched() == 0
        # freshly allocated empty tensors (torch hands out a NULL data_ptr() for them)
        out = runtime.gemm(torch.empty(2, 0, K, dtype=dt, device=DEV), W.view, resid=torch.empty(2, 0, N, device=DEV))
        assert out.shape == (2, 0, N)
        fn = lib.ispk_gemm_bf16 if dt == torch.bfloat16 else lib.ispk_gemm_f32
        assert fn(A.flat.data_ptr(), K, W.flat.data_ptr(), K, C.flat.data_ptr(), N, None, None, 0, None, 0, N, K, 0, 0, 0,
                  None) == 0
    assert lib.ispk_gemm_f32_batched(A.flat.data_ptr(), K, 0, W.flat.data_ptr(), K, 0, C.flat.data_ptr(), N, 0, 3, 0, N, K,
                                     None) == 0
    torch.cuda.synchronize()
    assert C.outside_touched() == 0


# --------------------------------------------------------------------------------------------- ispk_gemm_f32_batched
@pytest.mark.parametrize("batch,M,N,K", [(3, 100, 72, 64), (4, 300, 200, 384), (2, 1, 8, 8)])
def test_gemm_f32_batched_strided(batch, M, N, K):
    """C[z] = A[z] W[z]^T with operand batch strides larger than the packed size and ldc > N (the attention backward's
    per-head products): every batch item against float64, nothing written outside the C views."""
    lib = runtime.lib()
    lda, ldw, ldc = K + 8, K + 4, N + 5
    sa, sw, sc = M * lda + 12, N * ldw + 4, M * ldc + 7
    a = synth._normal(f"t/glb/a{batch}{M}{K}", (batch, M, K))
    w = synth._normal(f"t/glb/w{batch}{N}{K}", (batch, N, K), K ** -0.5)
    Abuf = torch.full((batch * sa + SLACK,), float("nan"), device=DEV)
    Wbuf = torch.full((batch * sw + SLACK,), float("nan"), device=DEV)
    for z in range(batch):
        torch.as_strided(Abuf, (M, K), (lda, 1), z * sa).copy_(a[z].to(DEV))
        torch.as_strided(Wbuf, (N, K), (ldw, 1), z * sw).copy_(w[z].to(DEV))
    C = Buf(torch.float32, batch * sc // ldc + 1, ldc, ldc, 0)
    idx = (torch.arange(batch)[:, None, None] * sc + torch.arange(M)[None, :, None] * ldc +
           torch.arange(N)[None, None, :]).reshape(-1)
    outs = []
    for _ in range(2):
        C.reset()
        rc = lib.ispk_gemm_f32_batched(Abuf.data_ptr(), lda, sa, Wbuf.data_ptr(), ldw, sw, C.flat.data_ptr(), ldc, sc, batch,
                                       M, N, K, None)
        torch.cuda.synchronize()
        assert rc == 0, _err()
        outs.append(C.bits())
    assert torch.equal(outs[0], outs[1])
    got = C.flat.cpu()[idx].reshape(batch, M, N).double()
    ref = a.double() @ w.double().transpose(1, 2)
    assert (got - ref).abs().max().item() < 2e-5
    assert C.outside_touched(idx) == 0
