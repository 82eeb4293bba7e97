"""Float64 references of the training step's loss, norm and optimizer kernels, written from each operation's definition
(no call into isp_tts_amd), plus the seeded inputs and the shape lists that tests/test_train_kernels_reference_host.py and
tests/test_gpu_train_kernels.py share.

Every `*_ref` takes a `dtype`: float64 is the reference; float32 evaluates THE SAME formula in fp32 torch on the CPU, which is
how the rounding noise of an fp32 evaluation is measured (`FP32_NOISE` below, re-measured and printed by the host test).
"""
import math

import torch

F64 = torch.float64

# ------------------------------------------------------------------------------------------------ comparison helpers


def rel_err(got, want) -> float:
    """max |got - want| relative to max |want| - the `_close` form of tests/test_gpu_train.py."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    if got.numel() == 0:
        return 0.0
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def close(got, want, tol, what=""):
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    e = rel_err(got, want)
    assert e <= tol, f"{what}: max |diff| / max |ref| = {e:.3e} (tol {tol:.3g})"


def same_bits(a, b) -> bool:
    """Bit equality (NaN payloads and the sign of zero included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def rand_mask(shape, seed, keep=0.7):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) < keep


# ------------------------------------------------------------------------------------------------ the norms


def _xhat(x, eps):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return xc * rstd, rstd


def _norm_dx(g, xhat, rstd):
    return rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def layernorm_bwd_ref(x, dy, gamma, mask, eps=1e-5, dtype=F64):
    """y = xhat * gamma + beta, then y *= mask[row].  x, dy [rows, D]; gamma [D] | None (= ones); mask bool [rows] | None.
    -> dx [rows, D], dgamma [D], dbeta [D]."""
    x, dy = x.to(dtype), dy.to(dtype)
    gy = dy if mask is None else dy * mask.to(dtype)[:, None]
    xhat, rstd = _xhat(x, eps)
    g = gy if gamma is None else gy * gamma.to(dtype)
    return _norm_dx(g, xhat, rstd), (gy * xhat).sum(0), gy.sum(0)


def adaln_bwd_ref(x, dy, scale, mask, eps=1e-5, dtype=F64):
    """y = xhat * scale_b + shift_b (xhat without affine), then y *= mask[b, l].  x, dy [B, L, D]; scale [B, D];
    mask bool [B, L] | None.  -> dx [B, L, D], dscale [B, D], dshift [B, D]."""
    x, dy = x.to(dtype), dy.to(dtype)
    gy = dy if mask is None else dy * mask.to(dtype)[:, :, None]
    xhat, rstd = _xhat(x, eps)
    g = gy * scale.to(dtype)[:, None, :]
    return _norm_dx(g, xhat, rstd), (gy * xhat).sum(1), gy.sum(1)


# ------------------------------------------------------------------------------------------------ time embedding


def time_features(t, inv_freq, freq_scale, dtype=F64):
    """f = [t, sin a, cos a] with the argument a rounded as the kernel rounds it, fp32(fp32(t * fs) * inv_freq), and only then
    promoted: at a ~ 1000 rad one fp32 rounding of `a` moves sin by ~6e-5, which is the input's precision, not the kernel's."""
    t32 = t.reshape(-1).float()
    a = ((t32[:, None] * freq_scale.float().reshape(1, 1)) * inv_freq.float().reshape(1, -1)).to(dtype)
    return torch.cat([t32.to(dtype)[:, None], torch.sin(a), torch.cos(a)], dim=1)


def time_embedding_fwd(f, w0, b0, w1, b1):
    """The forward over given features: h = silu(W0 f + b0), out = W1 h + b1 (the host test differentiates this)."""
    pre = f @ w0.T + b0
    return (pre * torch.sigmoid(pre)) @ w1.T + b1


def time_embedding_bwd_ref(t, inv_freq, freq_scale, w0, b0, w1, d_out, dtype=F64):
    """-> dw0 [E, 1 + 2H], db0 [E], dw1 [E, E], db1 [E] for d_out [n, E]; t gets no gradient."""
    f = time_features(t, inv_freq, freq_scale, dtype)
    w0, b0, w1, d_out = w0.to(dtype), b0.to(dtype), w1.to(dtype), d_out.reshape(f.shape[0], -1).to(dtype)
    pre = f @ w0.T + b0
    sg = 1.0 / (1.0 + torch.exp(-pre))
    h = pre * sg
    dpre = (d_out @ w1) * (sg * (1.0 + pre * (1.0 - sg)))
    return dpre.T @ f, dpre.sum(0), d_out.T @ h, d_out.sum(0)


# ------------------------------------------------------------------------------------------------ the losses


def flow_loss_bwd_ref(raw, flow, mask, grad_out=1.0, dtype=F64):
    """d/d raw of go * mean_b sum_{l, c} m (raw - flow)^2 / max(C n_b, 1e-5), n_b = valid rows of utterance b."""
    raw, flow, m = raw.to(dtype), flow.to(dtype), mask.to(dtype)
    B, L, C = raw.shape
    den = torch.clamp(C * m.sum(1), min=1e-5) * B
    return (2.0 * grad_out) * m[:, :, None] * (raw - flow) / den[:, None, None]


def mel_loss_ref(out, tgt, mel_len, grad_out=1.0, dtype=F64):
    """loss = mean_b sum_{c, t < len_b} (out - tgt)^2 / max(C len_b, 1e-5), len_b = clamp(mel_len_b, 0, T);
    -> (loss, grad_out * d loss / d out) - the loss itself is not scaled."""
    out, tgt = out.to(dtype), tgt.to(dtype)
    B, C, T = out.shape
    ln = mel_len.to(torch.int64).clamp(0, T)
    valid = (torch.arange(T)[None, :] < ln[:, None]).to(dtype)[:, None, :]
    den = torch.clamp((C * ln).to(dtype), min=1e-5)
    d = out - tgt
    loss = ((d * d * valid).sum((1, 2)) / den).sum() / B
    return loss, (2.0 * grad_out) * d * valid / (den * B)[:, None, None]


def mel_grad_rows_ref(dmel, mask):
    """[B, C, T] -> [B, T, C] rows times the 0/1 frame mask [B, T] (exact in any precision)."""
    g = dmel.transpose(1, 2)
    return (g if mask is None else g * mask.to(dmel.dtype)[:, :, None]).contiguous()


# ------------------------------------------------------------------------------------------------ the optimizer


def sqnorm_ref(g) -> float:
    return float((g.double() ** 2).sum())


def clip_coef(sqnorm: float, max_norm: float, grad_scale: float) -> float:
    """clamp(max_norm / (norm * grad_scale + 1e-6), max=1); a NaN norm propagates, an infinite one gives 0."""
    norm = math.sqrt(sqnorm) * grad_scale if sqnorm == sqnorm else float("nan")
    c = max_norm / (norm + 1e-6)
    return c if c != c else min(c, 1.0)


def adamw_ref(p, g, m, v, n_decay, lr, betas, eps, wd, step, sqnorm=None, max_norm=1.0, grad_scale=1.0, dtype=F64):
    """One AdamW step over flat arenas in the order documented above `adam_one` in csrc/train.hip (torch's
    _single_tensor_adamw); elements [0, n_decay) alone get the decay and the clip.  `sqnorm`: the squared norm of the decay
    group's UNSCALED gradients (a float), None = no clipping.  -> new (p, m, v)."""
    p, g, m, v = p.to(dtype).clone(), g.to(dtype) * grad_scale, m.to(dtype), v.to(dtype)
    if sqnorm is not None:
        g[:n_decay] = g[:n_decay] * clip_coef(float(sqnorm), max_norm, grad_scale)
    b1, b2 = betas
    p[:n_decay] = p[:n_decay] * (1.0 - lr * wd)
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = torch.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adam_factors(lr, betas, eps, wd, step, max_norm, grad_scale):
    """The ten factors of ispk_adam_args_t in Python float64 (decay_mul, 1-b1, b2, 1-b2, lr/bc1, 1/sqrt(bc2), sqrt(bc2), eps,
    max_norm, grad_scale), not yet rounded."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return [1.0 - lr * wd, 1.0 - b1, b2, 1.0 - b2, lr / bc1, 1.0 / math.sqrt(bc2), math.sqrt(bc2), eps, max_norm, grad_scale]


# ------------------------------------------------------------------------------------------------ shapes and seeded inputs

ADALN_SHAPES = [(3, 50, 256), (2, 7, 384), (1, 16, 256), (2, 17, 384), (1, 40, 384)]
TIME_SHAPES = [(3, 32, 32), (64, 32, 32), (65, 32, 32), (130, 32, 32), (70, 79, 64), (5, 1, 1)]
FLOW_CASES = [((5, 37, 3), (37, 1, 0, 20, 36)), ((2, 300, 3), (300, 0)), ((2, 300, 3), (1, 257)), ((1, 1, 1), (1,)), ((1, 1, 1), (0,))]
MEL_CASES = [((4, 80, 300), (0, 1, 300, 309)), ((2, 5, 7), (16, 0)), ((2, 5, 7), (1, 7))]
MEL_ROWS_SHAPES = [(2, 80, 203), (3, 5, 33), (1, 33, 31)]
LN_DIMS = [256, 384]
LN_ROWS = [1, 63, 64, 65, 513, 2113]
SQNORM_SIZES = [0, 1, 3, 4, 1027, 1024 * 256 * 4 + 5]
ADAMW_SIZES = [(7, 0), (7, 7), (1030, 513), (1030, 1029), (4096 * 256 * 4 + 6, 1_000_001)]
# (name, sqnorm | None, grad_scale) with max_norm = 1: norm * grad_scale = 3 -> clip 1/3 (active), 0.5 -> idle
ADAMW_VARIANTS = [("noclip", None, 1.0), ("active", 9.0, 1.0), ("idle", 0.25, 1.0), ("scaled_active", 147456.0, 1.0 / 128),
                  ("scaled_noclip", None, 1.0 / 128), ("inf", float("inf"), 1.0), ("nan", float("nan"), 1.0)]
ADAMW_HYPER = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-2)
ADAMW_STEPS = 3


def adaln_inputs(B, L, D, masked):
    """x, dy [B, L, D]; a wide [B, 3 D + 5] conditioning tensor whose columns 5 .. 5 + D are `scale`; mask [B, L] | None with
    every row of the LAST utterance masked when B > 1."""
    x, dy = rand((B, L, D), 101, 2.0) + 0.3, rand((B, L, D), 102)
    wide = 1.0 + 0.3 * rand((B, 3 * D + 5), 103)
    mask = None
    if masked:
        mask = rand_mask((B, L), 104)
        mask[0, 0], mask[0, L - 1] = True, False
        if B > 1:
            mask[B - 1] = False
    return x, dy, wide, mask


def time_inputs(n, H, E):
    """t in [0, 1] with exact 0 and 1; the model's frequencies (theta = 1000, freq_scale = 1000: arguments up to 1000 rad)."""
    g = torch.Generator().manual_seed(111)
    t = torch.rand((n,), generator=g)
    t[0], t[n - 1] = 0.0, 1.0
    inv_freq = 1000.0 ** -(torch.arange(H).float() / H)
    K0 = 1 + 2 * H
    return dict(t=t, inv_freq=inv_freq, freq_scale=torch.full((1,), 1000.0), w0=rand((E, K0), 112, K0 ** -0.5), b0=rand((E,), 113, 0.1),
                w1=rand((E, E), 114, E ** -0.5), d_out=rand((n, E), 115))


def flow_inputs(shape, lens):
    B, L, C = shape
    mask = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    return rand(shape, 121), rand(shape, 122), mask


def mel_inputs(shape):
    return rand(shape, 131), rand(shape, 132)


def ln_inputs(rows, dim):
    """x, dy, gamma, base (what dx holds before an accumulating call), mask_drop (last row masked), mask_keep (last row kept)."""
    x, dy = rand((rows, dim), 141, 2.0) + 0.3, rand((rows, dim), 142)
    gamma, base = 1.0 + 0.1 * rand((dim,), 143), rand((rows, dim), 144)
    drop = rand_mask((rows,), 145)
    drop[rows - 1] = False
    keep = rand_mask((rows,), 146)
    keep[rows - 1] = True
    return x, dy, gamma, base, drop, keep


def adamw_inputs(n):
    """p, m, v (non-zero moments, as after earlier steps) and one gradient per step."""
    p, m = rand((n,), 151), rand((n,), 152, 0.02)
    v = rand((n,), 153, 0.02) ** 2 + 1e-6
    return p, m, v, [rand((n,), 160 + s, 0.03) for s in range(ADAMW_STEPS)]


def adamw_run(p, m, v, grads, n_decay, sqnorm, grad_scale, dtype=F64):
    """ADAMW_STEPS steps of adamw_ref carrying p, m, v; the gradients are divided by grad_scale first, so that every variant
    updates with gradients of the same size."""
    p, m, v = p.to(dtype), m.to(dtype), v.to(dtype)
    h = ADAMW_HYPER
    for s, g in enumerate(grads):
        p, m, v = adamw_ref(p, g / grad_scale, m, v, n_decay, h["lr"], h["betas"], h["eps"], h["wd"], s + 1, sqnorm, 1.0, grad_scale, dtype)
    return p, m, v


# ------------------------------------------------------------------------------------------------ fp32 noise
# max over the GPU shapes of rel_err(fp32 evaluation on the CPU, float64 reference), per kernel output: measured by
# tests/test_train_kernels_reference_host.py::test_fp32_noise_table (which prints the per-shape figures and fails when an
# entry here is more than a factor 2 from what it measures).  A kernel is allowed 8 x its figure, and never more than 1e-4.
FP32_NOISE = {
    "adaln_bwd.dx": 1.62e-7, "adaln_bwd.dscale": 1.48e-7, "adaln_bwd.dshift": 1.77e-7,
    "time_embedding_bwd.dw0": 4.60e-7, "time_embedding_bwd.db0": 3.01e-7, "time_embedding_bwd.dw1": 3.73e-7,
    "time_embedding_bwd.db1": 1.16e-7,
    "flow_loss_bwd.d_raw": 8.81e-8,
    "adamw.p": 2.92e-7, "adamw.m": 1.06e-7, "adamw.v": 1.99e-7,
}
TOL_CAP = 1e-4
LAYERNORM_TOL = 2e-5      # tests/test_gpu_train.py::test_layernorm_backward
MEL_LOSS_TOL = 2e-6       # tests/test_gpu_train.py::test_mel_loss_value_and_gradient


def tol(key: str) -> float:
    return min(8.0 * FP32_NOISE[key], TOL_CAP)


def measure_fp32_noise() -> dict:
    """key -> {shape label: rel_err of the fp32 evaluation} over every GPU shape of the kernels without a project tolerance."""
    out: dict = {k: {} for k in FP32_NOISE}

    def put(kernel, names, label, lo, hi):
        for name, a, b in zip(names, lo, hi):
            out[f"{kernel}.{name}"][label] = rel_err(a, b)

    for B, L, D in ADALN_SHAPES:
        for masked in (False, True):
            x, dy, wide, mask = adaln_inputs(B, L, D, masked)
            args = (x, dy, wide[:, 5:5 + D], mask)
            put("adaln_bwd", ("dx", "dscale", "dshift"), f"{(B, L, D)}{' masked' if masked else ''}",
                adaln_bwd_ref(*args, dtype=torch.float32), adaln_bwd_ref(*args))
    for shape in TIME_SHAPES:
        i = time_inputs(*shape)
        put("time_embedding_bwd", ("dw0", "db0", "dw1", "db1"), f"{shape}", time_embedding_bwd_ref(**i, dtype=torch.float32),
            time_embedding_bwd_ref(**i))
    for shape, lens in FLOW_CASES:
        raw, flow, mask = flow_inputs(shape, lens)
        for go in (1.0, 0.37):
            put("flow_loss_bwd", ("d_raw",), f"{shape} lens {lens} go {go}", (flow_loss_bwd_ref(raw, flow, mask, go, torch.float32),),
                (flow_loss_bwd_ref(raw, flow, mask, go),))
    for n, n_decay in ADAMW_SIZES:
        p, m, v, grads = adamw_inputs(n)
        for name, sq, gs in ADAMW_VARIANTS:
            if sq is not None and sq != sq:
                continue        # NaN norm: the decay group is NaN in both, nothing to measure
            put("adamw", ("p", "m", "v"), f"{(n, n_decay)} {name}", adamw_run(p, m, v, grads, n_decay, sq, gs, torch.float32),
                adamw_run(p, m, v, grads, n_decay, sq, gs))
    return out
