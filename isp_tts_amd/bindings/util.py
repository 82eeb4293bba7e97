"""Data movement (csrc/util.hip): staging, segment copies, fills, small element-wise passes."""
import ctypes
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["_Segment", "SEG_COPY", "SEG_ADD", "SEG_BF16", "_Stage", "stage_weights", "segments", "cat0", "deliver_grads", "zero_",
           "_zero_rows", "zeros", "scale_", "sum_scalars", "exp_pad", "sqrt_scale", "copy2d", "permute021", "conv_weight_flip",
           "draw_seed"]


class _Segment(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", ctypes.c_int64), ("mode", ctypes.c_int32)]


SEG_COPY, SEG_ADD, SEG_BF16 = 0, 1, 2


class _Stage(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("ld_dst", ctypes.c_int64), ("flags", ctypes.c_int32)]


def stage_weights(items) -> None:
    """ispk_stage_weights: items = [(src fp32 contiguous [rows, cols], dst 2-D view with unit column stride (fp32 or bf16),
    transposed: bool, exp: bool)], 16 per launch.  dst is [rows, cols], or [cols, rows] when transposed."""
    if not items:
        return
    _rt.stage_calls += 1
    arr = (_Stage * len(items))()
    nbytes = 0.0
    for k, (src, dst, tr, ex) in enumerate(items):
        _rt._dev(src, dst)
        src = src.detach()
        assert src.dtype == torch.float32 and src.ndim == 2 and src.is_contiguous() and dst.ndim == 2 and dst.stride(1) == 1
        assert tuple(dst.shape) == ((src.shape[1], src.shape[0]) if tr else tuple(src.shape)) and dst.dtype in (torch.float32, torch.bfloat16)
        arr[k].src, arr[k].dst, arr[k].rows, arr[k].cols = src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1]
        arr[k].ld_dst = dst.stride(0)
        arr[k].flags = (1 if tr else 0) | (2 if dst.dtype == torch.bfloat16 else 0) | (4 if ex else 0)
        nbytes += src.numel() * (4.0 + dst.element_size())
    _rt._launch("stage_kernel", 0.0, nbytes, _rt.lib().ispk_stage_weights, ctypes.cast(arr, ctypes.c_void_p), len(items), _rt._stream())


def segments(items) -> None:
    """ispk_segments_f32: items = [(src fp32 contiguous, dst contiguous view, mode)], any number, 32 per launch:
    SEG_COPY dst = src, SEG_ADD dst += src, SEG_BF16 dst(bf16) = src."""
    if not items:
        return
    arr = (_Segment * len(items))()
    nbytes = 0.0
    for k, (src, dst, mode) in enumerate(items):
        _rt._dev(src, dst)
        assert src.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
        assert dst.dtype == (torch.bfloat16 if mode == SEG_BF16 else torch.float32)
        arr[k].src, arr[k].dst, arr[k].n, arr[k].mode = src.data_ptr(), dst.data_ptr(), src.numel(), mode
        nbytes += src.numel() * (4.0 + dst.element_size() * (2 if mode == SEG_ADD else 1))
    _rt._launch("segments_kernel", 0.0, nbytes, _rt.lib().ispk_segments_f32, ctypes.cast(arr, ctypes.c_void_p), len(items), _rt._stream())


def cat0(tensors, dtype: torch.dtype = torch.float32) -> Tensor:
    """torch.cat(tensors, 0).to(dtype) of contiguous fp32 tensors as one ispk_segments_f32 launch (weights that change every
    training step: the fused [to_q; to_kv] image, the adaptive norms' stacked projections)."""
    srcs = [t.detach() for t in tensors]
    assert dtype in (torch.float32, torch.bfloat16) and all(t.dtype == torch.float32 and t.is_contiguous() for t in srcs)
    rows = sum(t.shape[0] for t in srcs)
    out = torch.empty((rows, *srcs[0].shape[1:]), dtype=dtype, device=srcs[0].device)
    items, r = [], 0
    for t in srcs:
        items.append((t, out[r:r + t.shape[0]], SEG_BF16 if dtype == torch.bfloat16 else SEG_COPY))
        r += t.shape[0]
    _rt.segments(items)
    return out


def deliver_grads(pairs) -> list:
    """pairs = [(parameter, gradient | None)] -> the list of gradients to hand to autograd.  A gradient whose parameter's .grad
    is a buffer of an optimizer arena (`FlatParameters` marks it `_ispk_grad_arena`) is written - or added, if something has
    been delivered since the arena was zeroed - into it by ONE segments launch for the whole list, and autograd gets None:
    no AccumulateGrad add per parameter."""
    out, items, seen = [], [], set()
    for p, g in pairs:
        if g is not None and not p.requires_grad:
            # frozen AFTER the arena was built (model.freeze(), row f3): autograd would have dropped this gradient - so do we,
            # instead of writing it into the arena where AdamW would apply it
            out.append(None)
            continue
        buf = p.grad if g is not None else None
        if buf is not None and getattr(buf, "_ispk_grad_arena", False) and g.is_cuda:
            g = g.detach()
            g = g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()
            if buf.data_ptr() in seen:
                # the same parameter twice in one call: two segments of ONE launch writing one buffer would race - flush first
                _rt.segments(items)
                items, seen = [], set()
            seen.add(buf.data_ptr())
            items.append((g, buf, SEG_ADD if getattr(buf, "_ispk_dirty", False) else SEG_COPY))
            buf._ispk_dirty = True
            out.append(None)
        else:
            out.append(g)
    _rt.segments(items)
    return out


def zero_(t: Tensor) -> Tensor:
    """ispk_fill_zero on a contiguous tensor."""
    _rt._dev(t)
    assert t.is_contiguous()
    _rt._launch("fill_zero_kernel", 0.0, float(t.numel() * t.element_size()), _rt.lib().ispk_fill_zero, t.data_ptr(),
                t.numel() * t.element_size(), _rt._stream())
    return t


def _zero_rows(out: Tensor) -> Tensor:
    """The result of a weight-gradient product over zero rows: `out` zeroed (a strided view: copied from a zeroed scratch)."""
    if out.numel() == 0 or out.is_contiguous():
        return _rt.zero_(out) if out.numel() else out
    z = _rt.zeros(tuple(out.shape[-2:]), device=out.device)
    for o in (out,) if out.ndim == 2 else out:
        _rt.copy2d(z, o)
    return out


def zeros(shape, dtype: torch.dtype = torch.float32, device=None) -> Tensor:
    return _rt.zero_(torch.empty(shape, dtype=dtype, device=device))


def scale_(x: Tensor, s_dev: Optional[Tensor] = None, s_host: float = 1.0) -> Tensor:
    """ispk_scale_f32: x *= s_dev[0] * s_host in place (s_dev: a one-element fp32 device tensor or None)."""
    _rt._dev(x, s_dev)
    assert x.dtype == torch.float32 and x.is_contiguous() and (s_dev is None or (s_dev.dtype == torch.float32 and s_dev.numel() == 1))
    _rt._launch("scale_kernel", 0.0, 8.0 * x.numel(), _rt.lib().ispk_scale_f32, x.data_ptr(), x.numel(), _rt._ptr(s_dev), float(s_host), _rt._stream())
    return x


def sum_scalars(terms, weights=None) -> Tensor:
    """ispk_sum_scalars_f32 -> 0-dim fp32: sum_i weights[i] * terms[i] (one-element fp32 device tensors), in index order."""
    terms = list(terms)
    _rt._dev(*terms)
    assert 1 <= len(terms) <= 8 and all(t.dtype == torch.float32 and t.numel() == 1 for t in terms)
    ptrs = (ctypes.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
    ws = (ctypes.c_float * len(terms))(*([1.0] * len(terms) if weights is None else [float(w) for w in weights]))
    out = torch.empty((1,), dtype=torch.float32, device=terms[0].device)
    _rt._launch("sum_scalars_kernel", 0.0, 0.0, _rt.lib().ispk_sum_scalars_f32, ctypes.cast(ptrs, ctypes.c_void_p),
                ctypes.cast(ws, ctypes.c_void_p), len(terms), out.data_ptr(), _rt._stream())
    return out.reshape(())


def exp_pad(src: Tensor, total: Optional[int] = None) -> Tensor:
    """ispk_exp_pad_f32: exp(src) (fp32, flattened), zero-padded to `total` elements."""
    _rt._dev(src)
    src = src.detach().reshape(-1)
    assert src.dtype == torch.float32 and src.is_contiguous()
    total = src.numel() if total is None else total
    out = torch.empty((total,), dtype=torch.float32, device=src.device)
    _rt._launch("unary_kernel", 0.0, 0.0, _rt.lib().ispk_exp_pad_f32, src.data_ptr(), out.data_ptr(), src.numel(), total, _rt._stream())
    return out


def sqrt_scale(src: Tensor, scale: float = 1.0) -> Tensor:
    """ispk_sqrt_scale_f32: sqrt(src) * scale (fp32)."""
    _rt._dev(src)
    assert src.dtype == torch.float32 and src.is_contiguous()
    out = torch.empty_like(src)
    _rt._launch("unary_kernel", 0.0, 0.0, _rt.lib().ispk_sqrt_scale_f32, src.data_ptr(), out.data_ptr(), src.numel(), float(scale), _rt._stream())
    return out


def copy2d(src: Tensor, dst: Tensor) -> Tensor:
    """ispk_copy2d_f32: dst[:, :] = src for 2-D fp32 views with unit column stride."""
    _rt._dev(src, dst)
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.ndim == 2 and src.shape == dst.shape
    assert src.stride(1) == 1 and dst.stride(1) == 1
    _rt._launch("copy2d_kernel", 0.0, 8.0 * src.numel(), _rt.lib().ispk_copy2d_f32, src.data_ptr(), src.stride(0), dst.data_ptr(),
                dst.stride(0), src.shape[0], src.shape[1], _rt._stream())
    return dst


def permute021(src: Tensor) -> Tensor:
    """ispk_permute021_f32: [A, B, C] fp32 contiguous -> contiguous [A, C, B]."""
    _rt._dev(src)
    src = src.detach()
    assert src.dtype == torch.float32 and src.ndim == 3 and src.is_contiguous()
    A, B, C = src.shape
    out = torch.empty((A, C, B), dtype=torch.float32, device=src.device)
    _rt._launch("permute021_kernel", 0.0, 8.0 * src.numel(), _rt.lib().ispk_permute021_f32, src.data_ptr(), out.data_ptr(), A, B, C, _rt._stream())
    return out


def conv_weight_flip(w: Tensor) -> Tensor:
    """ispk_conv_weight_flip_f32: Conv1d weight [O, C, K] -> [C, K * O] with wf[c][(K-1-k) O + o] = w[o][c][k]."""
    _rt._dev(w)
    w = w.detach()
    assert w.dtype == torch.float32 and w.ndim == 3 and w.is_contiguous()
    O, C, K = w.shape
    out = torch.empty((C, K * O), dtype=torch.float32, device=w.device)
    _rt._launch("conv_flip_kernel", 0.0, 8.0 * w.numel(), _rt.lib().ispk_conv_weight_flip_f32, w.data_ptr(), out.data_ptr(), O, C, K, _rt._stream())
    return out


def draw_seed() -> int:
    """A 62-bit seed for one launch group's dropout masks from torch's CPU generator (`torch.manual_seed(s)` reproduces a
    run): a host-side draw, no device tensor and no device round trip."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())
