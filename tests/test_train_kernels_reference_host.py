"""The float64 references of tests/train_kernels_reference.py against torch autograd (float64, over the forward
expression) and torch.optim.AdamW + clip_grad_norm_; agreement is to float64 rounding.  Also measures and prints the
fp32-noise figures from which tests/test_gpu_train_kernels.py takes the tolerances of the kernels that had none.  CPU only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_kernels_reference as R

TOL = 1e-10


@pytest.mark.parametrize("rows,dim,masked,affine", [(65, 256, True, True), (7, 384, False, True), (33, 384, True, False)])
def test_layernorm_bwd_ref_matches_autograd(rows, dim, masked, affine):
    x, dy, gamma, _, drop, _ = R.ln_inputs(rows, dim)
    mask = drop if masked else None
    x64 = x.double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), torch.zeros(dim, dtype=torch.float64, requires_grad=True)
    y = F.layer_norm(x64, (dim,), g64 if affine else None, None, 1e-5)
    y = y + b64
    if masked:
        y = y * mask[:, None]
    y.backward(dy.double())
    dx, dg, db = R.layernorm_bwd_ref(x, dy, gamma if affine else None, mask)
    R.close(dx, x64.grad, TOL, "dx")
    R.close(db, b64.grad, TOL, "dbeta")
    if affine:
        R.close(dg, g64.grad, TOL, "dgamma")
    else:
        ones = torch.ones(dim, dtype=torch.float64, requires_grad=True)
        y1 = F.layer_norm(x.double(), (dim,), ones, None, 1e-5)
        (y1 * mask[:, None] if masked else y1).backward(dy.double())
        R.close(dg, ones.grad, TOL, "dgamma of a unit weight")


@pytest.mark.parametrize("B,L,D,masked", [(3, 50, 256, True), (2, 7, 384, True), (1, 40, 384, False)])
def test_adaln_bwd_ref_matches_autograd(B, L, D, masked):
    x, dy, wide, mask = R.adaln_inputs(B, L, D, masked)
    x64 = x.double().requires_grad_()
    scale = wide[:, 5:5 + D].double().requires_grad_()
    shift = wide[:, 5 + D:5 + 2 * D].double().requires_grad_()
    y = F.layer_norm(x64, (D,), None, None, 1e-5) * scale[:, None, :] + shift[:, None, :]
    if masked:
        y = y * mask[:, :, None]
    y.backward(dy.double())
    dx, dscale, dshift = R.adaln_bwd_ref(x, dy, wide[:, 5:5 + D], mask)
    R.close(dx, x64.grad, TOL, "dx")
    R.close(dscale, scale.grad, TOL, "dscale")
    R.close(dshift, shift.grad, TOL, "dshift")
    if masked and B > 1:
        assert float(dscale[B - 1].abs().max()) == 0.0 and float(dshift[B - 1].abs().max()) == 0.0


@pytest.mark.parametrize("n,H,E", [(3, 32, 32), (70, 79, 64), (5, 1, 1)])
def test_time_embedding_bwd_ref_matches_autograd(n, H, E):
    i = R.time_inputs(n, H, E)
    f = R.time_features(i["t"], i["inv_freq"], i["freq_scale"])
    assert f.dtype == torch.float64 and f.shape == (n, 1 + 2 * H)
    # the argument is the fp32 product, promoted: sin / cos of exactly that number
    a32 = (i["t"] * i["freq_scale"]) * i["inv_freq"][H - 1]
    assert a32.dtype == torch.float32 and torch.equal(f[:, H], torch.sin(a32.double())) and torch.equal(f[:, 2 * H], torch.cos(a32.double()))
    w0, b0, w1 = (i[k].double().requires_grad_() for k in ("w0", "b0", "w1"))
    b1 = torch.zeros(E, dtype=torch.float64, requires_grad=True)
    R.time_embedding_fwd(f, w0, b0, w1, b1).backward(i["d_out"].double())
    for name, got, want in zip(("dw0", "db0", "dw1", "db1"), R.time_embedding_bwd_ref(**i), (w0.grad, b0.grad, w1.grad, b1.grad)):
        R.close(got, want, TOL, name)


@pytest.mark.parametrize("shape,lens", R.FLOW_CASES)
@pytest.mark.parametrize("go", [1.0, 0.37])
def test_flow_loss_bwd_ref_matches_autograd(shape, lens, go):
    raw, flow, mask = R.flow_inputs(shape, lens)
    B, L, C = shape
    r64 = raw.double().requires_grad_()
    m = mask.double()
    per = ((r64 * m[:, :, None] - flow.double() * m[:, :, None]) ** 2).sum((1, 2)) / torch.clamp(C * m.sum(1), min=1e-5)
    (go * per.mean()).backward()
    got = R.flow_loss_bwd_ref(raw, flow, mask, go)
    R.close(got, r64.grad, TOL, "d raw")
    assert bool(torch.isfinite(got).all())
    for b, n in enumerate(lens):
        assert float(got[b, n:].abs().max() if n < L else 0.0) == 0.0


@pytest.mark.parametrize("shape,lens", R.MEL_CASES)
def test_mel_loss_ref_matches_autograd(shape, lens):
    out, tgt = R.mel_inputs(shape)
    B, C, T = shape
    o64 = out.double().requires_grad_()
    total = 0.0
    for b, n in enumerate(lens):      # utterance by utterance, the clamp written out
        n = min(max(n, 0), T)
        total = total + ((o64[b, :, :n] - tgt[b, :, :n].double()) ** 2).sum() / max(C * n, 1e-5)
    loss = total / B
    (0.7 * loss).backward()
    got_loss, got_grad = R.mel_loss_ref(out, tgt, torch.tensor(lens), 0.7)
    R.close(got_loss, loss, TOL, "loss")
    R.close(got_grad, o64.grad, TOL, "d out")


def test_mel_grad_rows_ref():
    d, mask = R.rand((3, 5, 33), 1), R.rand_mask((3, 33), 2)
    got = R.mel_grad_rows_ref(d, mask)
    assert got.shape == (3, 33, 5) and got.is_contiguous()
    for b in range(3):
        for t in (0, 17, 32):
            assert torch.equal(got[b, t], d[b, :, t] * float(mask[b, t]))
    assert torch.equal(R.mel_grad_rows_ref(d, None), d.transpose(1, 2))


def test_sqnorm_ref():
    g = R.rand((1027,), 3)
    assert R.sqnorm_ref(g) == pytest.approx(math.fsum(float(x) ** 2 for x in g), rel=1e-14)
    assert R.sqnorm_ref(g[:0]) == 0.0


@pytest.mark.parametrize("n,n_decay", [(7, 0), (7, 7), (1030, 513)])
@pytest.mark.parametrize("gscale,grad_scale", [(0.03, 1.0), (3.0, 1.0), (3.0, 1.0 / 128)])
def test_adamw_ref_matches_torch_optim(n, n_decay, gscale, grad_scale):
    """torch.optim.AdamW over two groups (decay / none), clip_grad_norm_ on group 0 only, 3 steps in float64, with the clip
    idle (gradients of 0.03) and active (3.0); adamw_ref gets the squared norm of the UNSCALED decay gradients."""
    h = R.ADAMW_HYPER
    p0, m0, v0, _ = R.adamw_inputs(n)
    a = torch.nn.Parameter(p0[:n_decay].double().clone())
    b = torch.nn.Parameter(p0[n_decay:].double().clone())
    opt = torch.optim.AdamW([dict(params=[a], weight_decay=h["wd"]), dict(params=[b], weight_decay=0.0)], lr=h["lr"], betas=h["betas"],
                            eps=h["eps"])
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    active = []
    for step in range(1, 4):
        g = R.rand((n,), 170 + step, gscale / grad_scale)
        a.grad, b.grad = g[:n_decay].double() * grad_scale, g[n_decay:].double() * grad_scale
        active.append(float(a.grad.norm()) > 1.0)
        torch.nn.utils.clip_grad_norm_([a], 1.0)
        opt.step()
        p, m, v = R.adamw_ref(p, g, m, v, n_decay, h["lr"], h["betas"], h["eps"], h["wd"], step, R.sqnorm_ref(g[:n_decay]), 1.0, grad_scale)
        R.close(p, torch.cat([a.detach(), b.detach()]), TOL, f"p, step {step}")
        for ref_t, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
            R.close(ref_t, torch.cat([opt.state[a][key], opt.state[b][key]]), TOL, f"{key}, step {step}")
    if n_decay >= 513:      # the clip was idle on every step / active on every step, as the case means it
        assert active == [gscale == 3.0] * 3


def test_adamw_ref_edges():
    """No clipping = a clip of 1; an infinite norm = a zero gradient in the decay group; a NaN norm turns that group, and only
    it, NaN."""
    h = R.ADAMW_HYPER
    p, m, v, (g, *_) = R.adamw_inputs(1030)
    args = (513, h["lr"], h["betas"], h["eps"], h["wd"], 2)
    for a, b in zip(R.adamw_ref(p, g, m, v, *args), R.adamw_ref(p, g, m, v, *args, 0.25, 1.0, 1.0)):
        assert torch.equal(a, b)
    g0 = g.clone()
    g0[:513] = 0.0
    for a, b in zip(R.adamw_ref(p, g, m, v, *args, float("inf")), R.adamw_ref(p, g0, m, v, *args)):
        assert torch.equal(a, b)
    for t in R.adamw_ref(p, g, m, v, *args, float("nan")):
        assert bool(torch.isnan(t[:513]).all()) and bool(torch.isfinite(t[513:]).all())
    assert R.clip_coef(9.0, 1.0, 1.0) == 1.0 / (3.0 + 1e-6) and R.clip_coef(0.0, 1.0, 1.0) == 1.0
    assert R.clip_coef(147456.0, 1.0, 1.0 / 128) == 1.0 / (3.0 + 1e-6) and R.clip_coef(float("inf"), 1.0, 1.0) == 0.0


def test_adam_factors():
    f = R.adam_factors(2e-3, (0.9, 0.999), 1e-8, 1e-2, 3, 1.0, 0.5)
    assert f[0] == 1.0 - 2e-5 and f[2] == 0.999 and f[4] == 2e-3 / (1 - 0.9 ** 3) and f[5] * f[6] == pytest.approx(1.0, rel=1e-15)
    assert f[7:] == [1e-8, 1.0, 0.5]
    # the C entry points take float arguments: the betas are rounded BEFORE 1 - beta is formed, so those factors sit this far
    # (relative) from the ones of the unrounded hyper-parameters; the GPU test's float64 reference uses the unrounded ones
    r32 = lambda x: float(np.float32(x))      # noqa: E731
    g = R.adam_factors(r32(2e-3), (r32(0.9), r32(0.999)), r32(1e-8), r32(1e-2), 3, 1.0, 0.5)
    worst = max(abs(a - b) / abs(a) for a, b in zip(f, g))
    print(f"\nAdamW factors, float arguments against double arguments: worst relative distance {worst:.3e}")
    assert worst < 2e-5


def test_fp32_noise_table():
    """Measures what an fp32 evaluation of each formula loses against float64 at every GPU shape, prints it, and holds the
    recorded figures of train_kernels_reference.FP32_NOISE (max over the shapes) within a factor 2 of the measurement."""
    measured = R.measure_fp32_noise()
    print("\nfp32 evaluation on the CPU against float64, max |diff| / max |ref|")
    for key, per_shape in measured.items():
        worst = max(per_shape.values())
        print(f"  {key:28s} measured {worst:.3e}  recorded {R.FP32_NOISE[key]:.3e}  -> tolerance {R.tol(key):.3e}")
        for label, e in per_shape.items():
            print(f"      {label:60s} {e:.3e}")
    for key, per_shape in measured.items():
        worst = max(per_shape.values())
        assert worst / 2 <= R.FP32_NOISE[key] <= worst * 2, f"{key}: recorded {R.FP32_NOISE[key]:.3e}, measured {worst:.3e}"
        assert R.tol(key) <= R.TOL_CAP
