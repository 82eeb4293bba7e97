"""The fused feed-forward kernels (csrc/ffn.hip: ispk_ffn_bf16, ispk_ffn_bf16_prenorm, ispk_ffn_pack_w2_bf16; csrc/ffn2.hip:
ispk_ffn_bf16_prenorm2, ispk_attn_out_ffn_bf16 / _norm_bf16 / _qkv_bf16, ispk_ffn_bf16_prenorm2_split,
ispk_attn_out_ffn_split_bf16, ispk_ffn_combine_ln_f32, ispk_ffn_chunk_w2_bf16, ispk_chunk_k16_bf16), each against its float64
reference (tests/ffn_reference.py, proved against plain PyTorch and against its mutants by tests/test_ffn_reference_host.py) at
the smallest shapes that reach every tile edge, pipeline length, stride, mask pattern and flag.

How a case runs.  `_direct` calls the C entry with every output in a sentinel-filled buffer with guard rows behind row R (and,
strided, guard columns beside the row) and checks afterwards that the guards and the inputs are untouched and no output is NaN;
where the `runtime` wrapper can express the case (`_wrapper`: everything but ldo / ld_qkv / ld_ln / part_stride, the flag sets
attn_out_ffn does not expose and the combine pass alone) the wrapper's result must have the same bits - which is also the "second
call, same bits" check.

Branches per entry point, and the cases that reach them (R rows; inner = 32 x chunks)
  every eight-wave entry (a workgroup owns 128 rows; LayerNorm prologue 16 rows per wave; row groups of 32; epilogue 64 rows a
  pass, 32 with the q/kv epilogue; three-stage pipeline over the chunks, DMA chunk indices clamped at both ends)
    R = 1                 one live row: every other row of the tile is the clamped row 0, never stored
    R = 16, 17            the LayerNorm prologue's wave edge        R = 32, 33     a row group's edge (33: group 1 has one row)
    R = 64, 65            the epilogue's pass edge (q/kv: every second pass)     R = 127, 128, 129   the tile edge; a second workgroup
    R = 257               three workgroups; with mask `tile` the middle one has no valid row
    inner 32 (prenorm2)   1 chunk: the pipeline's three iterations each run ONE stage      inner 64    2 chunks: never all three stages
    inner 96, 128, 160    3 (the depth), 4, 5 chunks: one, two, three steady-state iterations     inner 1536  the production size
  ispk_ffn_bf16_prenorm2          flags 0 / MASK_OUT / MASK_ACC / both; statistics
  ispk_attn_out_ffn_bf16          MASK_ACC masks the projection's operand rows, MASK_OUT the rows; statistics
  ispk_attn_out_ffn_norm_bf16     fp32 / bf16 LayerNorm output, ln_mask 0 / 1 (also with flags 0: the row mask then belongs to the
                                  LayerNorm alone), out stored / NULL
  ispk_attn_out_ffn_qkv_bf16      the 32-row passes; q/kv of masked rows (LN_next of a zero row = beta)
  ispk_ffn_bf16_prenorm2_split / ispk_attn_out_ffn_split_bf16 + ispk_ffn_combine_ln_f32     (R, inner, splits)
    (129, 64, 1) one split of the minimum two chunks     (129, 128, 2), (1, 128, 2) two of two     (17, 192, 3), (129, 192, 2) 2 / 3 each
    (257, 1536, 24) two each, 72 workgroups              (130, 1536, 16) three each
  ispk_ffn_combine_ln_f32 alone   rows 1, 7, 8, 9, 257 (8 rows per workgroup) x splits 1, 2, 3, 16 x residual given / NULL x mask
                                  none / prefix x LayerNorm none / fp32 / bf16 x ln_mask 0 / 1; y bit for bit
  ispk_ffn_bf16 / ispk_ffn_bf16_prenorm (ffn_bf16_kernel<KC, B1, PK, EP, ST, LN, LX>, KC = dim / 64; 4 waves x 32 rows)
    R = 1, 31, 32, 33, 127, 128, 129 at inner 96; inner 64, 96, 160 at R = 129; both dims; at EVERY shape the nine instances:
    <KC, 0, 1, hot>          packed W2, MASK_OUT + residual            <KC, 0, 1, dyn>        packed, bias2 + MASK_ACC
    <KC, 0, 0, dyn>          row-major W2, no residual, no mask        <KC, 1, 1, dyn>        bias1 + bias2, packed
    <KC, 1, 0, dyn>          bias1, row-major, both mask flags
    <KC, 0, 1, hot, LX>      pre-norm                                  <KC, 0, 1, hot, LN, LX>   pre-norm with statistics
    <KC, 0, 1, dyn, LX>      pre-norm with bias2                       <KC, 0, 1, dyn, LN, LX>   pre-norm, bias2, statistics, no mask
  Before this module only <6, 0, 1, hot>, <6, 0, 1, hot, LX>, <6, 0, 1, hot, LN, LX>, <4, 0, 1, dyn>, <4, 0, 1, hot, LX> (+ LN) and
  <6, 0, 1, dyn, LX> (unmasked) were run, each at one or two shapes.
  Flags and masks: every entry at (129, 96) with the patterns ones / prefix / zeros, and at (257, 160) with `tile`, under every
  flag set it permits; `none` with flags 0.

What the new cases found: ispk_attn_out_ffn_norm_bf16 with ln_mask = 1 and NO mask flag left the masked rows of ln_out
unmasked (the epilogue read the row mask only under MASK_ACC / MASK_OUT; the wrapper always sets both, so the model never saw
it).  Fixed in csrc/ffn2.hip; the six cases `attn_out_ffn[ln_mask,norm_*] ... flags=0` with masks prefix / tile / zeros show it.

Measured on an MI355X (947 cases, 5 s): the worst ratio of each figure to its allowance, over all cases of an entry point
(<= 1 passes; FACTOR = 3.0 and RMS_FACTOR = 1.5 did not have to move)
    entry point               out|y max   out|y rms   parts max / rms   stats mean / rstd   ln      qkv max / rms
    ffn_fused                 0.333       0.978
    ffn_prenorm               0.333       0.972                         0.241 / 0.014
    ffn_prenorm2              0.343       0.880                         0.257 / 0.013
    attn_out_ffn              0.367       0.857
    attn_out_ffn + stats      0.367       0.857                         0.268 / 0.015
    attn_out_ffn + norm fp32  0.367       0.857                                             0.029
    attn_out_ffn + norm bf16  0.367       0.857                                             0.475
    attn_out_ffn + qkv        0.367       0.857                                                     0.333 / 0.667
    split                     0.378       0.877       0.421 / 0.698                         0.373
    split_proj                0.359       0.871       0.459 / 0.701                         0.406
    combine_ln alone          (y exact)                                                     0.010 fp32, 0.421 bf16
  0.333 / 0.667 = the kernel's error IS the rounded evaluation's (the same bf16 roundings decide it).  The rms figures above 0.7
  are all at R < 128 under mask `prefix`: there e_round comes from the 128-row extension, 50 of whose rows are masked (error 0),
  while the first R <= 50 rows are all valid - the allowance is diluted by sqrt(78 / 128), and R = 1 is the one row 0 against the
  average row (0.978 at dim 256, inner 96).  At R >= 128 the worst rms ratio is 0.68.
"""
import functools

import pytest
import torch

import ffn_reference as R
from isp_tts_amd import runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = {F32: (torch.int32, 0x7FC0BEEF), BF16: (torch.int16, 0x7FC1)}      # NaN bit patterns
PAD, OFF = 16, 8            # a strided operand is the column slice [OFF, OFF + width) of rows of width + PAD elements
GUARD_ROWS = 3
CASES = R.all_cases()
MAIN_CASES = R.cases4() + R.cases2() + R.cases_split()
WORST = {}


def entry_key(c):
    if c.entry == "attn_out_ffn":
        for v in ("stats", "norm_f32", "norm_bf16", "qkv"):
            if c.has(v):
                return f"attn_out_ffn+{v}"
    return c.entry


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the worst ratio of each figure to its allowance, per entry point (shown with -s)."""
    yield
    for (e, what), ratio in sorted(WORST.items()):
        print(f"\nworst {e:24s} {what:12s} {ratio:.3f}", end="")


def _record(c, r):
    for what, ratio in r.items():
        what = "part.max" if what.startswith("part") and what.endswith("max") else "part.rms" if what.startswith("part") else what
        k = (entry_key(c), what)
        WORST[k] = max(WORST.get(k, 0.0), ratio)


# ------------------------------------------------------------------------------------------------ buffers


class Out:
    """rows x width elements at row stride ld inside a sentinel-filled buffer with GUARD_ROWS rows and 16 elements behind them."""

    def __init__(self, rows, width, dt, ld=None):
        self.rows, self.width, self.dt, self.ld = rows, width, dt, ld or width
        self.ib, self.sent = SENT[dt]
        self.back = torch.empty(((rows + GUARD_ROWS) * self.ld + 16,), dtype=dt, device=DEV)
        self.back.view(self.ib).fill_(self.sent)

    def ptr(self):
        return self.back.data_ptr()

    @property
    def mat(self):
        return self.back[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    def guards_intact(self):
        b = self.back.view(self.ib).clone()
        b[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.width] = self.sent
        return bool((b == self.sent).all())

    def cpu(self):
        return self.mat.cpu().contiguous()


class In:
    """A device operand: contiguous, or (strided) a column slice of NaN-padded rows.  `unchanged()` compares the whole backing."""

    def __init__(self, t, dt, strided=False):
        t = t.to(dt)
        if strided and t.dim() == 2:
            self.back = torch.full((t.shape[0], t.shape[1] + PAD), float("nan"), dtype=dt, device=DEV)
            self.back[:, OFF:OFF + t.shape[1]] = t.to(DEV)
            self.t = self.back[:, OFF:OFF + t.shape[1]]
        else:
            self.back = t.to(DEV).contiguous()
            self.t = self.back
        self.before = self.back.clone()

    def ptr(self):
        return self.t.data_ptr()

    @property
    def ld(self):
        return self.t.stride(0)

    def unchanged(self):
        ib = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[self.back.element_size()]
        return torch.equal(self.back.view(ib), self.before.view(ib))


@functools.lru_cache(maxsize=None)
def _weights(dim, inner):
    """The (dim, inner) set's weights on the device, staged once through the wrappers (test_weight_staging checks those exactly)."""
    i = R.inputs(dim, inner)
    w = {k: i[k].to(DEV) for k in ("g", "b", "bias1", "bias2", "fg", "fb")}
    w["w1"], w2 = i["w1"].to(BF16).to(DEV), i["w2"].to(BF16).to(DEV)
    w["w2"], w["w2p"], w["w2c"] = w2, runtime.ffn_pack_w2(w2), runtime.ffn_chunk_w2(w2)
    if dim == 384:
        w["woc"], w["wqc"] = runtime.ffn_chunk_w2(i["wo"].to(BF16).to(DEV)), runtime.chunk_k16(i["wq"].to(BF16).to(DEV))
    w["w2s"] = In(i["w2"], BF16, strided=True)         # row-major W2 with ldw2 = inner + PAD
    return w


def _ok(rc, what):
    assert rc == 0, f"{what}: {rc} {runtime.lib().ispk_last_error_string()!r}"


# ------------------------------------------------------------------------------------------------ one call


def _direct(c, rows=None, strided=False, x=None, o=None):
    """The case through the C entry points, `rows` rows (default c.R), operands and outputs strided or not; x / o replace the
    fp32 rows / the attention output.  -> {name: CPU tensor}; guards, inputs and NaN-freedom are asserted here."""
    lib, st = runtime.lib(), runtime._stream()
    n, D, Fi = c.R if rows is None else rows, c.dim, c.inner
    i, w = R.inputs(D, Fi), _weights(D, Fi)
    mask_cpu = R.mask_pattern(c.mask, n)
    mask = None if mask_cpu is None else In(mask_cpu, torch.bool)
    mp = None if mask is None else mask.ptr()
    ld = D + PAD if strided else D
    ins, outs, res = [mask] if mask is not None else [], {}, {}
    xs = In(i["x"][:n] if x is None else x, F32, strided)
    ins.append(xs)
    main = "y" if c.entry in R.SPLIT_ENTRIES else "out"
    if not c.has("noout"):
        outs[main] = Out(n, D, F32, ld)
    op = None if c.has("noout") else outs[main].ptr()
    if c.has("stats"):
        outs["stats"] = Out(n, 2, F32)
    sp = outs["stats"].ptr() if c.has("stats") else None
    nbf = c.has("norm_bf16")
    if nbf or c.has("norm_f32"):
        outs["ln"] = Out(n, D, BF16 if nbf else F32, ld)
    lp = outs["ln"].ptr() if "ln" in outs else None
    b2 = w["bias2"].data_ptr() if c.has("bias2") else None
    if c.entry in R.PROJ_ENTRIES:
        os_ = In(i["o"][:n] if o is None else o, BF16, strided)
        ins.append(os_)
    if c.entry == "ffn_fused":
        xb = In(i["xb"][:n], BF16, strided)
        rs = None if c.has("noresid") else In(i["resid"][:n], F32, strided)
        ins += [xb] + ([rs] if rs is not None else [])
        if c.has("rowmajor"):
            w2, ldw2 = (w["w2s"].ptr(), w["w2s"].ld) if strided else (w["w2"].data_ptr(), Fi)
        else:
            w2, ldw2 = w["w2p"].data_ptr(), 0
        _ok(lib.ispk_ffn_bf16(xb.ptr(), xb.ld, w["w1"].data_ptr(), D, w["bias1"].data_ptr() if c.has("bias1") else None, w2, ldw2, b2,
                              None if rs is None else rs.ptr(), 0 if rs is None else rs.ld, mp, op, ld, n, D, Fi, c.flags, st), c.label)
    elif c.entry == "ffn_prenorm":
        _ok(lib.ispk_ffn_bf16_prenorm(xs.ptr(), xs.ld, w["g"].data_ptr(), w["b"].data_ptr(), R.EPS, w["w1"].data_ptr(), D, w["w2p"].data_ptr(),
                                      b2, mp, op, ld, n, D, Fi, c.flags, sp, R.EPS, st), c.label)
    elif c.entry == "ffn_prenorm2":
        _ok(lib.ispk_ffn_bf16_prenorm2(xs.ptr(), xs.ld, w["g"].data_ptr(), w["b"].data_ptr(), R.EPS, w["w1"].data_ptr(), w["w2c"].data_ptr(),
                                       mp, op, ld, n, D, Fi, c.flags, sp, R.EPS, st), c.label)
    elif c.entry == "attn_out_ffn":
        head = (xs.ptr(), xs.ld, os_.ptr(), os_.ld, w["woc"].data_ptr(), w["g"].data_ptr(), w["b"].data_ptr(), R.EPS, w["w1"].data_ptr(),
                w["w2c"].data_ptr(), mp, op, ld, n, D, Fi, c.flags)
        if "ln" in outs:
            _ok(lib.ispk_attn_out_ffn_norm_bf16(*head, w["fg"].data_ptr(), w["fb"].data_ptr(), R.EPS, int(c.has("ln_mask")), lp, ld, int(nbf), st),
                c.label)
        elif c.has("qkv"):
            outs["qkv"] = Out(n, R.NQ, BF16, R.NQ + PAD if strided else R.NQ)
            _ok(lib.ispk_attn_out_ffn_qkv_bf16(*head, w["fg"].data_ptr(), w["fb"].data_ptr(), R.EPS, w["wqc"].data_ptr(), outs["qkv"].ptr(),
                                               outs["qkv"].ld, st), c.label)
        else:
            _ok(lib.ispk_attn_out_ffn_bf16(*head, sp, R.EPS, st), c.label)
    else:
        stride = n * D + (4 * 33 if strided else 0)
        outs["parts"] = Out(c.splits, n * D, F32, stride)
        pp = outs["parts"].ptr()
        if c.entry == "split_proj":
            _ok(lib.ispk_attn_out_ffn_split_bf16(xs.ptr(), xs.ld, os_.ptr(), os_.ld, w["woc"].data_ptr(), w["g"].data_ptr(), w["b"].data_ptr(), R.EPS,
                                                 w["w1"].data_ptr(), w["w2c"].data_ptr(), mp, c.flags, pp, stride, c.splits, n, D, Fi, st), c.label)
        else:
            _ok(lib.ispk_ffn_bf16_prenorm2_split(xs.ptr(), xs.ld, w["g"].data_ptr(), w["b"].data_ptr(), R.EPS, w["w1"].data_ptr(), w["w2c"].data_ptr(),
                                                 pp, stride, c.splits, n, D, Fi, st), c.label)
        _ok(lib.ispk_ffn_combine_ln_f32(None if c.entry == "split_proj" else xs.ptr(), xs.ld, pp, stride, c.splits, mp, op, ld,
                                        w["fg"].data_ptr() if lp else None, w["fb"].data_ptr() if lp else None, R.EPS, int(c.has("ln_mask")), lp, ld,
                                        int(nbf), n, D, st), c.label)
    torch.cuda.synchronize()
    for name, ob in outs.items():
        assert ob.guards_intact(), f"{c.label}: wrote outside {name} ({'strided' if strided else 'contiguous'}, {n} rows)"
        res[name] = ob.cpu().view(c.splits, n, D) if name == "parts" else ob.cpu()
    for t in ins:
        assert t.unchanged(), f"{c.label}: an input changed"
    if x is None and o is None:
        for name, t in res.items():
            assert not bool(torch.isnan(t.float()).any()), f"{c.label}: NaN in {name}"
    return res


def _expressible(c):
    """Whether the `runtime` wrapper of the entry can make this call."""
    if c.entry == "attn_out_ffn":
        return c.flags == (0 if c.mask == "none" else R.MASK_ACC | R.MASK_OUT)
    if c.entry == "split_proj":
        return c.flags == (0 if c.mask == "none" else R.MASK_ACC)
    return True


def _wrapper(c, rows=None, strided=False):
    """The case through the runtime wrappers (x, attn_out, resid and row-major W2 may be views)."""
    n, D, Fi = c.R if rows is None else rows, c.dim, c.inner
    i, w = R.inputs(D, Fi), _weights(D, Fi)
    m = R.mask_pattern(c.mask, n)
    m = None if m is None else m.to(DEV)
    x = In(i["x"][:n], F32, strided).t
    res = {}
    if c.entry == "ffn_fused":
        w2 = (w["w2s"].t if strided else w["w2"]) if c.has("rowmajor") else w["w2p"]
        res["out"] = runtime.ffn_fused(In(i["xb"][:n], BF16, strided).t, w["w1"], w2, None if c.has("noresid") else In(i["resid"][:n], F32, strided).t,
                                       m, w["bias1"] if c.has("bias1") else None, w["bias2"] if c.has("bias2") else None, c.flags)
    elif c.entry in ("ffn_prenorm", "ffn_prenorm2"):
        kw = dict(mask=m, flags=c.flags, norm_eps=R.EPS, want_stats=c.has("stats"), stats_eps=R.EPS)
        r = (runtime.ffn_prenorm(x, w["g"], w["b"], w["w1"], w["w2p"], bias2=w["bias2"] if c.has("bias2") else None, **kw)
             if c.entry == "ffn_prenorm" else runtime.ffn_prenorm2(x, w["g"], w["b"], w["w1"], w["w2c"], **kw))
        res["out"], res["stats"] = r if c.has("stats") else (r, None)
    elif c.entry == "attn_out_ffn":
        o = In(i["o"][:n], BF16, strided).t
        args = (x, o, w["woc"], w["g"], w["b"], w["w1"], w["w2c"])
        if c.has("norm_f32") or c.has("norm_bf16"):
            fn = (w["fg"], w["fb"], R.EPS, c.has("ln_mask"), BF16 if c.has("norm_bf16") else F32)
            res["out"], res["ln"] = runtime.attn_out_ffn(*args, mask=m, norm_eps=R.EPS, final_norm=fn, want_out=not c.has("noout"))
        elif c.has("qkv"):
            res["out"], res["qkv"] = runtime.attn_out_ffn(*args, mask=m, norm_eps=R.EPS, next_qkv=(w["fg"], w["fb"], R.EPS, w["wqc"]))
        else:
            r = runtime.attn_out_ffn(*args, mask=m, norm_eps=R.EPS, want_stats=c.has("stats"), stats_eps=R.EPS)
            res["out"], res["stats"] = r if c.has("stats") else (r, None)
    else:
        nn_ = None
        if c.has("norm_f32") or c.has("norm_bf16"):
            nn_ = (w["fg"], w["fb"], R.EPS, c.has("ln_mask"), BF16 if c.has("norm_bf16") else F32)
        proj = (In(i["o"][:n], BF16, strided).t, w["woc"]) if c.entry == "split_proj" else None
        res["y"], res["ln"] = runtime.ffn_prenorm2_split(x, w["g"], w["b"], w["w1"], w["w2c"], m, c.splits, next_norm=nn_, norm_eps=R.EPS, attn_proj=proj)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items() if v is not None}


def _same(a, b, what, rows=None):
    """Bit equality of every output both calls have (the first `rows` rows)."""
    for k in a:
        if k not in b:
            continue
        x, y = a[k], b[k]
        if rows is not None:
            x, y = (x[:, :rows], y[:, :rows]) if k == "parts" else (x[:rows], y[:rows])
        assert _bits_equal(x, y), f"{what}: {k} differs in {int((x.float() != y.float()).sum())} elements"


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _with_rows(c, got):
    """A call that does not store its rows is judged with the rows of the call that does (its LayerNorm output has the same bits)."""
    if not c.has("noout"):
        return got
    full = _direct(R.Case(c.entry, c.R, c.inner, c.mask, c.flags, c.dim, tuple(o for o in c.opts if o != "noout"), c.splits))
    assert _bits_equal(full["ln"], got["ln"]), f"{c.label}: the LayerNorm output depends on whether the rows are stored"
    return {**got, "out": full["out"]}


# ------------------------------------------------------------------------------------------------ values


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.label.replace(" ", "_"))
def test_values_guards_and_a_second_call(c):
    got = _direct(c)
    again = _wrapper(c) if _expressible(c) else _direct(c)
    _same(got, again, f"{c.label}: second call ({'wrapper' if _expressible(c) else 'direct'})")
    judged = _with_rows(c, got)
    r = R.ratios(c, judged)
    print(f"{c.label}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    _record(c, r)
    assert R.masked_rows_are_zero(c, judged), f"{c.label}: a masked row is not zero"
    assert max(r.values()) <= 1.0, f"{c.label}: {r}"
    if c.entry in R.SPLIT_ENTRIES:      # y = the fp32 sum of the kernel's own parts in split order, times the mask: bit for bit
        x = None if c.entry == "split_proj" else R.inputs(c.dim, c.inner)["x"][:c.R].numpy()
        want = R.combine_f32(x, got["parts"].numpy(), R.mask_pattern(c.mask, c.R))
        assert want.tobytes() == got["y"].numpy().tobytes(), f"{c.label}: y is not x + p0 + p1 + ... in split order"


@pytest.mark.parametrize("c", MAIN_CASES, ids=lambda c: c.label.replace(" ", "_"))
def test_same_bits_strided_and_with_rows_appended(c):
    base = _direct(c)
    _same(base, _direct(c, strided=True), f"{c.label}: strided operands and outputs")
    if _expressible(c):
        _same(base, _wrapper(c, strided=True), f"{c.label}: strided operands through the wrapper")
    for k in (1, 130):
        _same(base, _direct(c, rows=c.R + k), f"{c.label}: {k} rows appended", rows=c.R)
    if c.entry == "ffn_fused":          # packed W2 against row-major W2
        opts = tuple(sorted(set(c.opts) ^ {"rowmajor"}))
        _same(base, _direct(R.Case(c.entry, c.R, c.inner, c.mask, c.flags, c.dim, opts)), f"{c.label}: packed against row-major W2")


LEAK_CASES = [c for c in R.flag_cases() if c.mask in ("prefix", "tile") or (c.mask == "zeros" and c.entry in R.PROJ_ENTRIES and c.flags & R.MASK_ACC)]


@pytest.mark.parametrize("c", LEAK_CASES, ids=lambda c: c.label.replace(" ", "_"))
def test_masked_rows_do_not_leak(c):
    """Masked rows of the attention output holding NaN, Inf or other numbers leave every output bit unchanged (MASK_ACC: they
    are not multiplied); other finite values in a masked row of x leave the other rows' bits unchanged."""
    i = R.inputs(c.dim, c.inner)
    mask = R.mask_pattern(c.mask, c.R)
    base = _direct(c)
    if c.entry in R.PROJ_ENTRIES and c.flags & R.MASK_ACC:
        for junk in (float("nan"), float("inf"), -3.0e38, 7.5):
            o = i["o"][:c.R].clone()
            o[~mask] = junk
            got = _direct(c, o=o)
            _same(base, got, f"{c.label}: {junk} in the masked rows of attn_out")
    if c.entry != "ffn_fused" and bool(mask.any()):
        x = i["x"][:c.R].clone()
        x[~mask] = 7.0 - 2.0 * x[~mask]
        got = _direct(c, x=x)
        for k in base:
            a, b = (base[k][:, mask], got[k][:, mask]) if k == "parts" else (base[k][mask], got[k][mask])
            assert _bits_equal(a, b), f"{c.label}: {k} of the valid rows changed with a masked row's x"
            assert not bool(torch.isnan(got[k].float()).any()), f"{c.label}: NaN in {k}"


# ------------------------------------------------------------------------------------------------ the combine pass alone


@pytest.mark.parametrize("rows", R.COMBINE_ROWS)
def test_combine_ln_alone(rows):
    """y bit for bit (a fixed sequence of fp32 adds and one multiply); the LayerNorm output against float64 of that y; strided x,
    y, ln_out and parts (part_stride > rows * 384); guards; masked rows exactly zero."""
    lib, st, D = runtime.lib(), runtime._stream(), 384
    i = R.inputs(384, 96)
    fg, fb = i["fg"].to(DEV), i["fb"].to(DEV)
    for splits in R.COMBINE_SPLITS:
        parts_cpu = (torch.randn((splits, rows, D), generator=torch.Generator().manual_seed(900 + splits)) * 0.3).contiguous()
        for strided in (False, True):
            stride = rows * D + (4 * 33 if strided else 0)
            ld = D + PAD if strided else D
            pb = torch.full((splits, stride), float("nan"), dtype=F32, device=DEV)
            pb[:, :rows * D] = parts_cpu.view(splits, -1).to(DEV)
            for with_x in (True, False):
                xs = In(i["x"][:rows], F32, strided) if with_x else None
                for mname in ("none", "prefix"):
                    mask_cpu = R.mask_pattern(mname, rows)
                    mask = None if mask_cpu is None else mask_cpu.to(DEV)
                    for norm in (None, F32, BF16):
                        for ln_mask in ((0, 1) if norm is not None and mask is not None else (0,)):
                            what = f"combine rows={rows} splits={splits} strided={strided} x={with_x} mask={mname} ln={norm} ln_mask={ln_mask}"
                            y = Out(rows, D, F32, ld)
                            ln = None if norm is None else Out(rows, D, norm, ld)
                            _ok(lib.ispk_ffn_combine_ln_f32(None if xs is None else xs.ptr(), ld if xs is None else xs.ld, pb.data_ptr(), stride, splits,
                                                            None if mask is None else mask.data_ptr(), y.ptr(), ld, None if ln is None else fg.data_ptr(),
                                                            None if ln is None else fb.data_ptr(), R.EPS, ln_mask, None if ln is None else ln.ptr(), ld,
                                                            int(norm == BF16), rows, D, st), what)
                            torch.cuda.synchronize()
                            assert y.guards_intact() and (ln is None or ln.guards_intact()), what
                            assert xs is None or xs.unchanged(), what
                            got = y.cpu()
                            want = R.combine_f32(i["x"][:rows].numpy() if with_x else None, parts_cpu.numpy(), mask_cpu)
                            assert want.tobytes() == got.numpy().tobytes(), f"{what}: y"
                            if ln is not None:
                                ref = R.final_norm_ref(got.double(), i["fg"], i["fb"], mask_cpu, ln_mask, norm == BF16)
                                err = float((ln.cpu().double() - ref).abs().max())
                                tol = R.LN_TOL[norm == BF16] * max(1.0, float(ref.abs().max()))
                                k = ("combine_ln", "ln_bf16" if norm == BF16 else "ln_f32")
                                WORST[k] = max(WORST.get(k, 0.0), err / tol)
                                assert err <= tol, f"{what}: LayerNorm output {err:.3e} > {tol:.3e}"
                                if ln_mask and mask_cpu is not None and not bool(mask_cpu.all()):
                                    assert float(ln.cpu()[~mask_cpu].float().abs().max()) == 0.0, what


# ------------------------------------------------------------------------------------------------ weight staging, instances


@pytest.mark.parametrize("dim,inner", [(256, 32), (256, 96), (384, 64), (384, 1536)])
def test_weight_staging_w2(dim, inner):
    """ispk_ffn_pack_w2_bf16 and ispk_ffn_chunk_w2_bf16 against the index formulas, from a contiguous and a row-strided source."""
    w2 = torch.randn((dim, inner), generator=torch.Generator().manual_seed(dim + inner)).to(BF16)
    for strided in (False, True):
        src = In(w2, BF16, strided)
        assert src.ld == inner + (PAD if strided else 0)
        assert _bits_equal(runtime.ffn_pack_w2(src.t).cpu(), R.pack_w2_ref(w2)), (dim, inner, strided, "pack")
        assert _bits_equal(runtime.ffn_chunk_w2(src.t).cpu(), R.chunk_w2_ref(w2)), (dim, inner, strided, "chunk")
        assert src.unchanged()
    out = Out(inner // 32, dim * 32, BF16)          # guards behind the image
    _ok(runtime.lib().ispk_ffn_pack_w2_bf16(src.ptr(), src.ld, dim, inner, out.ptr(), runtime._stream()), "pack_w2")
    torch.cuda.synchronize()
    assert out.guards_intact() and _bits_equal(out.cpu().view(inner // 32, dim, 32), R.pack_w2_ref(w2))
    out = Out(inner // 32, dim * 32, BF16)
    _ok(runtime.lib().ispk_ffn_chunk_w2_bf16(src.ptr(), src.ld, dim, inner, out.ptr(), runtime._stream()), "chunk_w2")
    torch.cuda.synchronize()
    assert out.guards_intact() and _bits_equal(out.cpu().view(inner // 32, dim, 32), R.chunk_w2_ref(w2))


@pytest.mark.parametrize("N,K", [(1, 16), (3, 32), (512, 384)])
def test_weight_staging_k16(N, K):
    w = torch.randn((N, K), generator=torch.Generator().manual_seed(N + K)).to(BF16)
    for strided in (False, True):
        src = In(w, BF16, strided)
        assert _bits_equal(runtime.chunk_k16(src.t).cpu(), R.chunk_k16_ref(w)), (N, K, strided)
        out = Out(K // 16, N * 16, BF16)
        _ok(runtime.lib().ispk_chunk_k16_bf16(src.ptr(), src.ld, N, K, out.ptr(), runtime._stream()), "chunk_k16")
        torch.cuda.synchronize()
        assert out.guards_intact() and src.unchanged() and _bits_equal(out.cpu().view(K // 16, N, 16), R.chunk_k16_ref(w))


def test_case_list_reaches_every_instance_of_the_four_wave_kernel():
    """ffn_launch's dispatch restated (ffn_reference.ffn4_instance): the cases above run all nine instances of both dims - at
    every shape of the table - that can be reached without an environment knob."""
    want = {(kc, b1, pk, ep, ln, lx) for kc in (4, 6) for (b1, pk, ep, ln, lx) in [
        (False, True, "hot", True, True), (False, True, "dyn", True, True), (False, True, "hot", False, True), (False, True, "dyn", False, True),
        (False, True, "hot", False, False), (False, True, "dyn", False, False), (False, False, "dyn", False, False),
        (True, True, "dyn", False, False), (True, False, "dyn", False, False)]}
    reached = {}
    for c in CASES:
        if c.entry in ("ffn_fused", "ffn_prenorm"):
            reached.setdefault(R.case_instance(c), []).append(c)
    for inst in sorted(want):
        assert inst in reached, inst
        print(f"ffn_bf16_kernel<KC={inst[0]}, B1={inst[1]}, PK={inst[2]}, EP={inst[3]}, LN={inst[4]}, LX={inst[5]}>: {len(reached[inst])} cases, "
              f"{len({(c.R, c.inner) for c in reached[inst]})} shapes")
    assert set(reached) == want
    for kind in ("split", "split_proj", "ffn_prenorm2", "attn_out_ffn"):     # the five product modes of the eight-wave kernel
        assert any(c.entry == kind for c in CASES)
    assert any(c.has("qkv") for c in CASES)
