"""The training step's loss, norm and optimizer kernels, each against its float64 reference (tests/train_kernels_reference.py,
proved against autograd and torch.optim by tests/test_train_kernels_reference_host.py), through the `runtime` wrappers, at the
smallest shapes that reach every branch.

Branches per entry point
  ispk_adaln_bwd_f32 (adaln_bwd_kernel<D / 64, 16 waves>; one workgroup per utterance, wave w takes rows w, w + 16, ...)
    (3, 50, 256)  <4>; 50 rows: waves 0-1 take 4 rows, the others 3            (2, 7, 384)   <6>; 9 idle waves, LDS partials 0
    (1, 16, 256)  <4>; exactly one row per wave, one workgroup                 (2, 17, 384)  <6>; wave 0 alone takes 2 rows
    (1, 40, 384)  <6>; 8 waves with 3 rows, 8 with 2
    each with / without a row mask (last utterance fully masked when B > 1), add_to_dx on / off; scale, dscale, dshift are
    column slices of wider tensors (row stride != D).  A column order l * NPL + k instead of l + 64 k fails every shape.
  ispk_time_embedding_bwd_f32 (one workgroup, 64-value chunks, thread t owns outputs t, t + 1024, ... of [dW0 | dW1 | db0 | db1])
    (3, 32, 32)   one partial chunk, 3 slots per thread, some 4                (64, 32, 32)  one full chunk
    (65, 32, 32)  a second chunk of 1 value                                    (130, 32, 32) two full chunks and a tail of 2
    (70, 79, 64)  the documented maximum: 14400 outputs, 15 slots; chunk 2 has 6 values      (5, 1, 1)  6 outputs, 6 live threads
    `acc` reset per chunk would leave only the last chunk's terms: (65, ..), (130, ..), (70, ..) fail.  H = 80 / E = 65: refused.
  ispk_flow_loss_bwd_f32 (one workgroup per utterance, 256 threads count the valid rows first)
    (5, 37, 3) lengths 37, 1, 0, 20, 36;  (2, 300, 3) lengths (300, 0) and (1, 257): the count loop takes a second trip;
    (1, 1, 1) lengths 1 and 0; grad_out 1 and 0.37.  A zero-length utterance divides by 1e-5 and must still give exact zeros.
  ispk_mel_loss_f32 (one 1024-thread workgroup per utterance, then the mean): (4, 80, 300) with lengths 0, 1, T, T + 9 (clamped);
    (2, 5, 7): C T = 35 < 1024, most threads idle; grad_out 0.7.
  ispk_mel_grad_rows_f32 (32 x 32 tiles through LDS): (2, 80, 203) partial tiles in both directions, (3, 5, 33) one column tile
    of 5 and a second frame tile of 1, (1, 33, 31) the reverse; with / without the frame mask.
  ispk_layernorm_bwd_f32, dims 256 and 384, rows 1, 63, 64, 65, 513, 2113 = 1, 1, 1, 2, 9, 34 partials for
    layernorm_bwd_reduce_kernel, whose 8 groups add partials g, g + 8, ...: 1 and 2: groups 0 / 0-1 add one row in the tail loop;
    9: group 0 adds two; 34: every group takes the unrolled 4-row trip (p + 24 < nparts), groups 0-1 then one tail row.  Rows
    512, 2048, 2049 (8, 32, 33 partials: no tail row / the trip alone / group 0 alone goes on) run contiguous.  The workspace
    is filled with NaN before each call, so a partial read beyond `nparts` shows.
    contig      layernorm_bwd_vec_kernel<2 | 3>; odd rows: the last half-wave recomputes row rows-1 and must neither store nor sum
    vec_wide    the same kernel, operands and dx column slices [:, 4:4+dim] of [rows, dim + 8] (16-byte aligned, stride % 4 == 0)
    scalar_in   layernorm_bwd_kernel<4 | 6>: x and dy are slices [:, 1:1+dim] of [rows, dim + 3] (stride % 4 != 0, base misaligned)
    scalar_dx   layernorm_bwd_kernel<4 | 6>: contiguous operands, dx such a slice
    each: (gamma, no mask), (gamma=None, a mask that drops the last row), (a mask that keeps it, add_to_dx, no parameter gradients)
  ispk_layernorm_bwd_dual_f32: rows 1, 65, 513; bf16 copy == dx.to(bfloat16) bitwise, the fp32 results bitwise those of the
    plain entry; a misaligned operand is refused with code -4.
  ispk_grad_sqnorm_f32 (1024 x 256 float4 lanes per sweep, block 0 adds the n % 4 tail): n = 0 (NULL arena), 1 and 3 (tail only),
    4 (one float4), 1027 (257 float4 + 3), 1024 * 256 * 4 + 5 (a full sweep, a second trip of one float4, a tail of 1).
  ispk_adamw_f32 / ispk_adamw_f32_dev / ispk_adam_args_f32 (grid capped at 4096 blocks of 256 float4 lanes)
    (7, 0), (7, 7)  one float4 and a tail of 3 - dropping the (n & 3) tail leaves elements 4-6 untouched; no / all decay
    (1030, 513), (1030, 1029)  n_decay inside a float4 (513 = 4 * 128 + 1, 1029 = 4 * 257 + 1), tail of 2
    (4096 * 256 * 4 + 6, 1000001)  the capped grid loops twice, tail of 2
    variants: no clip; clip active (1/3) and idle; grad_scale 1/128 with and without clip; norm +inf (clip 0); norm NaN.

Tolerances (max |diff| / max |ref|).  layernorm_bwd keeps the 2e-5 of test_layernorm_backward and mel_loss the 2e-6 of
test_mel_loss_value_and_gradient.  The others had none: the same formula evaluated in fp32 torch on the CPU at every shape
above loses the figure below against float64 (max over the shapes; re-measured and printed per shape by
test_train_kernels_reference_host.py::test_fp32_noise_table), and the kernel is allowed 8 x that, capped at 1e-4.

    output                     fp32 noise   tolerance
    adaln_bwd dx               1.62e-7      1.30e-6
    adaln_bwd dscale           1.48e-7      1.18e-6
    adaln_bwd dshift           1.77e-7      1.42e-6
    time_embedding_bwd dw0     4.60e-7      3.68e-6
    time_embedding_bwd db0     3.01e-7      2.41e-6
    time_embedding_bwd dw1     3.73e-7      2.98e-6
    time_embedding_bwd db1     1.16e-7      9.28e-7
    flow_loss_bwd d_raw        8.81e-8      7.05e-7
    adamw p                    2.92e-7      2.34e-6
    adamw m                    1.06e-7      8.48e-7
    adamw v                    1.99e-7      1.59e-6

The AdamW reference uses the hyper-parameters as Python doubles.  The C entry points take them as floats, so 1 - beta is
formed from the rounded beta and sits up to 1.3e-5 (relative) from torch's factor; in p, m and v that is far below the
tolerances above.  `adam_args` is compared bit for bit with the factors computed in float64 from the float arguments.
"""
import functools

import numpy as np
import pytest
import torch

import train_kernels_reference as R
from isp_tts_amd import runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------ adaln_bwd


@pytest.mark.parametrize("add_to_dx", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,L,D", R.ADALN_SHAPES)
def test_adaln_bwd(B, L, D, masked, add_to_dx):
    x, dy, wide, mask = R.adaln_inputs(B, L, D, masked)
    want_dx, want_ds, want_dt = R.adaln_bwd_ref(x, dy, wide[:, 5:5 + D], mask)
    base, sentinel = R.rand((B, L, D), 105), R.rand((B, 2 * D + 9), 106)
    outside = torch.ones(2 * D + 9, dtype=torch.bool)
    outside[2:2 + D] = False
    outside[5 + D:5 + 2 * D] = False

    def run():
        wd, out = wide.to(DEV), sentinel.to(DEV)
        dx = runtime.adaln_bwd(x.to(DEV), dy.to(DEV), wd[:, 5:5 + D], _dev(mask), base.to(DEV) if add_to_dx else None, add_to_dx,
                               out[:, 2:2 + D], out[:, 5 + D:5 + 2 * D])
        assert R.same_bits(wd, wide)
        return dx.cpu(), out.cpu()

    dx, out = run()
    R.close(dx, want_dx + base.double() if add_to_dx else want_dx, R.tol("adaln_bwd.dx"), "dx")
    R.close(out[:, 2:2 + D], want_ds, R.tol("adaln_bwd.dscale"), "dscale")
    R.close(out[:, 5 + D:5 + 2 * D], want_dt, R.tol("adaln_bwd.dshift"), "dshift")
    assert R.same_bits(out[:, outside], sentinel[:, outside]), "columns outside the dscale / dshift slices were written"
    if masked:
        dropped = ~mask
        assert torch.equal(dx[dropped], base[dropped] if add_to_dx else torch.zeros_like(dx[dropped]))
        if B > 1:       # every row of the last utterance is masked
            assert float(out[B - 1, 2:2 + D].abs().max()) == 0.0 and float(out[B - 1, 5 + D:5 + 2 * D].abs().max()) == 0.0
    dx2, out2 = run()
    assert R.same_bits(dx, dx2) and R.same_bits(out, out2)


# ------------------------------------------------------------------------------------------------ time_embedding_bwd


@pytest.mark.parametrize("n,H,E", R.TIME_SHAPES)
def test_time_embedding_bwd(n, H, E):
    i = R.time_inputs(n, H, E)
    assert float(i["t"].min()) == 0.0 and float(i["t"].max()) == 1.0
    want = R.time_embedding_bwd_ref(**i)
    d = {k: t.to(DEV) for k, t in i.items()}
    got = runtime.time_embedding_bwd(**d)
    for name, g, w in zip(("dw0", "db0", "dw1", "db1"), got, want):
        R.close(g, w, R.tol(f"time_embedding_bwd.{name}"), name)
    for a, b in zip(got, runtime.time_embedding_bwd(**d)):
        assert R.same_bits(a, b)


@pytest.mark.parametrize("n,H,E", [(3, 80, 32), (3, 32, 65)])
def test_time_embedding_bwd_refuses_sizes_beyond_its_slots(n, H, E):
    d = {k: t.to(DEV) for k, t in R.time_inputs(n, H, E).items()}
    with pytest.raises(runtime.IspkError, match=r"rc=-2.*bad shape"):
        runtime.time_embedding_bwd(**d)


# ------------------------------------------------------------------------------------------------ flow_loss_bwd


@pytest.mark.parametrize("go", [1.0, 0.37])
@pytest.mark.parametrize("shape,lens", R.FLOW_CASES)
def test_flow_loss_bwd(shape, lens, go):
    raw, flow, mask = R.flow_inputs(shape, lens)
    got = runtime.flow_loss_bwd(raw.to(DEV), flow.to(DEV), mask.to(DEV), go).cpu()
    R.close(got, R.flow_loss_bwd_ref(raw, flow, mask, go), R.tol("flow_loss_bwd.d_raw"), "d raw")
    assert bool(torch.isfinite(got).all())
    assert float(got[~mask].abs().max() if bool((~mask).any()) else 0.0) == 0.0
    for b, n in enumerate(lens):
        if n == 0:
            assert float(got[b].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ mel_loss, mel_grad_rows


@pytest.mark.parametrize("shape,lens", R.MEL_CASES)
def test_mel_loss(shape, lens):
    B, C, T = shape
    out, tgt = R.mel_inputs(shape)
    ln = torch.tensor(lens)
    want_loss, want_grad = R.mel_loss_ref(out, tgt, ln, 0.7)
    loss, grad = runtime.mel_loss(out.to(DEV), tgt.to(DEV), ln.to(DEV), want_grad=True, grad_out=0.7)
    R.close(loss.reshape(()), want_loss, R.MEL_LOSS_TOL, "loss")
    R.close(grad, want_grad, R.MEL_LOSS_TOL, "d out")
    grad = grad.cpu()
    assert bool(torch.isfinite(grad).all())
    for b, n in enumerate(lens):
        if n < T:
            assert float(grad[b, :, max(n, 0):].abs().max()) == 0.0
    loss2, none = runtime.mel_loss(out.to(DEV), tgt.to(DEV), ln.to(DEV))
    assert none is None and R.same_bits(loss, loss2)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,C,T", R.MEL_ROWS_SHAPES)
def test_mel_grad_rows(B, C, T, masked):
    dmel = R.rand((B, C, T), 135)
    mask = R.rand_mask((B, T), 136) if masked else None
    got = runtime.mel_grad_rows(dmel.to(DEV), _dev(mask)).cpu()
    want = R.mel_grad_rows_ref(dmel, mask)
    assert got.shape == (B, T, C) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ layernorm_bwd

LN_LAYOUTS = ["contig", "vec_wide", "scalar_in", "scalar_dx"]


def _placed(t, how):
    """-> (holder on the device, [rows, dim] view of it holding t): how = None (contiguous), "vec" ([:, 4:4+dim] of a
    [rows, dim + 8] holder) or "scalar" ([:, 1:1+dim] of [rows, dim + 3]).  The rest of a holder is a seeded pattern."""
    rows, dim = t.shape
    if how is None:
        d = t.to(DEV)
        return d, d
    pad, off = (8, 4) if how == "vec" else (3, 1)
    holder = R.rand((rows, dim + pad), 147)
    holder[:, off:off + dim] = t
    holder = holder.to(DEV)
    return holder, holder[:, off:off + dim]


def _outside(holder, dim, how):
    off = 4 if how == "vec" else 1
    keep = torch.ones(holder.shape[1], dtype=torch.bool)
    keep[off:off + dim] = False
    return holder.cpu()[:, keep]


@pytest.mark.parametrize("layout", LN_LAYOUTS)
@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("dim", R.LN_DIMS)
def test_layernorm_bwd(dim, rows, layout):
    x, dy, gamma, base, drop, keep = R.ln_inputs(rows, dim)
    how_in = {"contig": None, "vec_wide": "vec", "scalar_in": "scalar", "scalar_dx": None}[layout]
    how_dx = {"contig": None, "vec_wide": "vec", "scalar_in": None, "scalar_dx": "scalar"}[layout]
    (_, xd), (_, dyd), gd = _placed(x, how_in), _placed(dy, how_in), gamma.to(DEV)
    if how_in == "scalar":
        assert xd.stride(0) % 4 != 0 or rows == 1
        assert xd.data_ptr() % 16 != 0
    tol = R.LAYERNORM_TOL

    def call(want, g, mask, add, want_param_grads):
        runtime.workspace(DEV, 1).fill_(float("nan"))
        holder, dx = _placed(base, how_dx)
        before = _outside(holder, dim, how_dx) if how_dx else None
        got = runtime.layernorm_bwd(xd, dyd, g, row_mask=_dev(mask), dx=dx if (how_dx or add) else None, add_to_dx=add,
                                    want_param_grads=want_param_grads)
        R.close(got[0], want[0] + base.double() if add else want[0], tol, "dx")
        if want_param_grads:
            R.close(got[1], want[1], tol, "dgamma")
            R.close(got[2], want[2], tol, "dbeta")
        else:
            assert got[1] is None and got[2] is None
        if how_dx:
            assert R.same_bits(_outside(holder, dim, how_dx), before), "dx holder written outside the slice"
        return got[0].cpu()

    call(R.layernorm_bwd_ref(x, dy, gamma, None), gd, None, False, True)
    dx = call(R.layernorm_bwd_ref(x, dy, None, drop), None, drop, False, True)
    assert float(dx[~drop].abs().max()) == 0.0          # masked rows, the last one among them
    call(R.layernorm_bwd_ref(x, dy, gamma, keep), gd, keep, True, False)


@pytest.mark.parametrize("rows", [512, 2048, 2049])
@pytest.mark.parametrize("dim", R.LN_DIMS)
def test_layernorm_bwd_reduce_tail(dim, rows):
    x, dy, gamma, _, _, keep = R.ln_inputs(rows, dim)
    runtime.workspace(DEV, 1).fill_(float("nan"))
    got = runtime.layernorm_bwd(x.to(DEV), dy.to(DEV), gamma.to(DEV), row_mask=keep.to(DEV))
    for name, g, w in zip(("dx", "dgamma", "dbeta"), got, R.layernorm_bwd_ref(x, dy, gamma, keep)):
        R.close(g, w, R.LAYERNORM_TOL, name)


@pytest.mark.parametrize("rows", [1, 65, 513])
@pytest.mark.parametrize("dim", R.LN_DIMS)
def test_layernorm_bwd_bf16_copy(dim, rows):
    x, dy, gamma, base, _, keep = R.ln_inputs(rows, dim)
    xd, dyd, gd, md = x.to(DEV), dy.to(DEV), gamma.to(DEV), keep.to(DEV)
    plain = runtime.layernorm_bwd(xd, dyd, gd, row_mask=md)
    dual = runtime.layernorm_bwd(xd, dyd, gd, row_mask=md, bf16_copy=True)
    want = R.layernorm_bwd_ref(x, dy, gamma, keep)
    for name, a, b, w in zip(("dx", "dgamma", "dbeta"), plain, dual, want):
        R.close(a, w, R.LAYERNORM_TOL, name)
        assert R.same_bits(a, b), f"{name} differs with the bf16 copy"
    assert dual[3].dtype == torch.bfloat16 and dual[3].shape == x.shape and R.same_bits(dual[3], dual[0].to(torch.bfloat16))
    acc = runtime.layernorm_bwd(xd, dyd, gd, row_mask=md, dx=base.to(DEV), add_to_dx=True, want_param_grads=False, bf16_copy=True)
    R.close(acc[0], want[0] + base.double(), R.LAYERNORM_TOL, "dx accumulated")
    assert acc[1] is None and R.same_bits(acc[3], acc[0].to(torch.bfloat16))


@pytest.mark.parametrize("dim", R.LN_DIMS)
def test_layernorm_bwd_bf16_copy_refuses_a_misaligned_operand(dim):
    x, dy, gamma, *_ = R.ln_inputs(65, dim)
    _, xd = _placed(x, "scalar")
    with pytest.raises(runtime.IspkError, match=r"rc=-4"):
        runtime.layernorm_bwd(xd, dy.to(DEV), gamma.to(DEV), bf16_copy=True)


# ------------------------------------------------------------------------------------------------ grad_sqnorm


@pytest.mark.parametrize("n", R.SQNORM_SIZES)
def test_grad_sqnorm(n):
    buf = R.rand((n + 8,), 181)
    g = buf.to(DEV)[4:4 + n]        # a slice that begins on a 16-byte boundary
    want = np.float32(R.sqnorm_ref(buf[4:4 + n]))
    got = runtime.grad_sqnorm(g)
    value = np.float32(got.item())
    print(f"n={n}: kernel {value!r} float32(float64 sum) {want!r}")
    if n == 0:
        assert value == 0.0
    else:       # fp64 accumulation, one rounding at the end: within one ulp of the rounded float64 sum
        assert value in (want, np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(0)))
    assert R.same_bits(got, runtime.grad_sqnorm(g))


# ------------------------------------------------------------------------------------------------ adamw, adamw_dev, adam_args


@functools.lru_cache(maxsize=1)
def _adamw_inputs(n):
    return R.adamw_inputs(n)


@pytest.mark.parametrize("name,sq,gs", R.ADAMW_VARIANTS)
@pytest.mark.parametrize("n,n_decay", R.ADAMW_SIZES)
def test_adamw_and_adamw_dev(n, n_decay, name, sq, gs):
    h = R.ADAMW_HYPER
    p, m, v, grads = _adamw_inputs(n)
    want = R.adamw_run(p, m, v, grads, n_decay, sq, gs)
    nan_norm = sq is not None and sq != sq
    # (a NaN norm: the rest group sees neither the clip nor the decay, so it steps as it does without clipping)
    unclipped = R.adamw_run(p, m, v, grads, n_decay, None, gs) if nan_norm else want
    host = [t.to(DEV) for t in (p, m, v)]
    dev = [t.clone() for t in host]
    sqd = None if sq is None else torch.tensor([sq], dtype=torch.float32).to(DEV)
    args_dev = torch.empty((10,), dtype=torch.float32, device=DEV)
    for s, g in enumerate(grads):
        gd = (g / gs).to(DEV)
        runtime.adamw(host[0], gd, host[1], host[2], n_decay, h["lr"], h["betas"], h["eps"], h["wd"], s + 1, sqd, 1.0, gs)
        args_dev.copy_(runtime.adam_args(h["lr"], h["betas"], h["eps"], h["wd"], s + 1, 1.0, gs))
        runtime.adamw_dev(dev[0], gd, dev[1], dev[2], n_decay, args_dev, sqd)
    host, dev = [t.cpu() for t in host], [t.cpu() for t in dev]
    for what, a, b, w, u in zip("pmv", host, dev, want, unclipped):
        assert R.same_bits(a, b), f"{what}: adamw_dev differs from adamw"
        if nan_norm:          # the decay group turns NaN, the rest steps as usual
            assert bool(torch.isnan(a[:n_decay]).all()) and bool(torch.isnan(w[:n_decay]).all()), f"{what}: decay group not NaN"
            assert bool(torch.isfinite(a[n_decay:]).all()) and torch.equal(w[n_decay:], u[n_decay:])
            # the tolerance is relative to the max of the WHOLE arena, as in every other variant (the rest group alone can
            # be a single small element): the NaN group is replaced by the unclipped reference's values on both sides
            filled = a.double()
            filled[:n_decay] = u[:n_decay]
            R.close(filled, u, R.tol(f"adamw.{what}"), what)
        else:
            assert bool(torch.isfinite(a).all())
            R.close(a, w, R.tol(f"adamw.{what}"), what)


@pytest.mark.parametrize("step", [1, 2, 3, 1000])
@pytest.mark.parametrize("max_norm,gs", [(1.0, 1.0), (0.3, 1.0 / 128)])
def test_adam_args(step, max_norm, gs):
    """The ten factors, computed in Python float64 from the float arguments the entry point receives and rounded once."""
    h = R.ADAMW_HYPER
    r32 = lambda x: float(np.float32(x))      # noqa: E731
    want = np.array(R.adam_factors(r32(h["lr"]), (r32(h["betas"][0]), r32(h["betas"][1])), r32(h["eps"]), r32(h["wd"]), step,
                                   r32(max_norm), r32(gs)), dtype=np.float64).astype(np.float32)
    got = runtime.adam_args(h["lr"], h["betas"], h["eps"], h["wd"], step, max_norm, gs)
    assert got.dtype == torch.float32 and got.shape == (10,)
    assert R.same_bits(got, torch.from_numpy(want)), f"{got.tolist()} vs {want.tolist()}"
