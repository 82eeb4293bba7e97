"""ctypes binding of libispk.so (the C ABI declared in include/ispk.h, which is read here for the argument types) and thin
tensor-level wrappers.  This file holds the loader, the launch profiler and the helpers; the wrappers live in
bindings/<family>.py and are imported at the bottom, so `runtime.<name>` reaches all of them.

PyTorch here is plumbing only: it owns device memory and the stream.  Every wrapper passes raw
`data_ptr()`s and the CURRENT torch stream to the library, so launches are ordered with torch ops and are
capturable in a HIP graph.  There is no CPU fallback anywhere: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Optional

import torch
from torch import Tensor

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libispk.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ispk.h")

EP_GELU, EP_SILU, EP_MASK_ACC, EP_MASK_OUT, EP_BIAS_ROW, EP_MASK_COL, EP_OUT_BF16, EP_RESID_BF16, EP_ROWS_T, EP_OUT_SPLIT = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512)

_P, _I32, _I64, _U32, _F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float
_U64, _F64 = ctypes.c_uint64, ctypes.c_double

_C_TYPES = {"int32_t": _I32, "int64_t": _I64, "uint32_t": _U32, "uint64_t": _U64, "float": _F32, "double": _F64,
            "ispk_stream_t": _P}
_C_RETURNS = {"int32_t": _I32, "const char*": ctypes.c_char_p}


class IspkError(RuntimeError):
    pass


def _parse_header(text: str) -> tuple[dict, dict, int]:
    """The `ispk_*` prototypes of a C header as (name -> argtypes, name -> restype) and its ISPK_ABI_VERSION.  Strict: a
    prototype or a type it cannot read raises, so a new C type joins the two maps above and never binds as something else."""
    version = re.search(r"^#define\s+ISPK_ABI_VERSION\s+(\d+)", text, flags=re.M)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments first: one may begin behind a #define
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    argtypes, restypes = {}, {}
    for stmt in text.split(";"):
        entry = re.search(r"\bispk_\w+(?=\s*\()", stmt)
        if entry is None:
            continue
        name = entry.group()
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\bispk_\w+\s*\(([^()]*)\)\s*", stmt)
        ret = m and " ".join(m.group(1).replace("*", "* ").split()).replace(" *", "*")
        if ret not in _C_RETURNS or name in argtypes:
            raise IspkError(f"{name}: not one prototype with a known return type: `{' '.join(stmt.split())}`")
        restypes[name], argtypes[name] = _C_RETURNS[ret], []
        for param in ([] if m.group(2).strip() in ("", "void") else m.group(2).split(",")):
            *ctype, pname = param.replace("*", " * ").split() or [""]
            if "*" in ctype and pname.isidentifier():
                argtypes[name].append(ctypes.c_char_p if ctype == ["char", "*"] else _P)
            elif " ".join(ctype) in _C_TYPES and pname.isidentifier():
                argtypes[name].append(_C_TYPES[" ".join(ctype)])
            else:
                raise IspkError(f"{name}: unknown argument type in `{' '.join(param.split())}`")
    if version is None:
        raise IspkError("no `#define ISPK_ABI_VERSION <n>`")
    return argtypes, restypes, int(version.group(1))


# include/ispk.h is the one place the ABI is written: the compiler holds the definitions to it (csrc/common.h includes it),
# and the argtypes / restype of every entry point and the version that lib() expects are read from it here
try:
    with open(HEADER_PATH) as _f:
        SIGNATURES, RESTYPES, ABI_VERSION = _parse_header(_f.read())
except OSError as e:
    raise IspkError(f"{HEADER_PATH} cannot be read ({e}): the bindings take their argument types from it") from e

_lib = None


def lib() -> ctypes.CDLL:
    """Loads libispk.so.  Fails loudly when it has not been built (`python -m isp_tts_amd.build`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IspkError(f"{LIB_PATH} is missing: the HIP extension was not built "
                            f"(run `python -m isp_tts_amd.build` or `__graft_entry__.build()`); there is no CPU fallback")
        handle = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = argtypes
            fn.restype = RESTYPES[name]
        if handle.ispk_abi_version() != ABI_VERSION:
            raise IspkError(f"libispk.so ABI version {handle.ispk_abi_version()} != {ABI_VERSION} (rebuild: python -m isp_tts_amd.build)")
        _lib = handle
    return _lib


class LaunchProfiler:
    """Optional per-launch timing with HIP events on the launch stream (used by bench.py for the roofline object).
    Each record: (kernel label, algorithmic FLOPs, algorithmic HBM bytes, start event, end event)."""

    def __init__(self):
        self.records = []

    def summary(self) -> dict:
        """label -> {launches, total_ms, avg_us, flops, bytes} (call after a device synchronise)."""
        out: dict = {}
        for label, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(label, {"launches": 0, "total_ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["total_ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        for d in out.values():
            d["avg_us"] = 1e3 * d["total_ms"] / d["launches"]
        return out


_profiler: Optional[LaunchProfiler] = None


def set_profiler(p: Optional[LaunchProfiler]) -> None:
    global _profiler
    _profiler = p


# epilogue instances launch_panel() in csrc/gemm.hip compiles: qkv (bf16 out), FFN1 (bf16 out + GELU), out-projection
# (mask-acc + residual), to_mel (ROWS_T + mask-out + bias)
_PANEL_EPS = (64, 65, 4 | (1 << 17), 256 | 8 | (1 << 16))


def _launch(label: str, flops: float, nbytes: float, fn, *args) -> None:
    if _profiler is None:
        _check(fn(*args), label)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn(*args)
    e1.record()
    _check(rc, label)
    if label == "gemm_bf16_kernel":   # resolve to the instance the library actually dispatched
        v = lib().ispk_gemm_bf16_last_variant()
        if v // 1000 == 1:   # panel kernel <KC, EP>: EP = the compile-time epilogue instance (-1: the generic one)
            ep = (args[13] & 0xffff) | ((1 << 16) if args[6] else 0) | ((1 << 17) if args[7] else 0)
            label = f"gemm_bf16_panel_kernel<{v % 1000},{ep if ep in _PANEL_EPS else -1}>"
        else:
            label = {2: f"gemm_bf16_wide_kernel<{(v % 1000) // 10},{v % 10}>",
                     3: f"gemm_bf16_kernel<{(v % 1000) // 10},{v % 10}>"}.get(v // 1000, label)
    elif label.startswith("gemm_tn_b16_kernel") and lib().ispk_gemm_tn_last_plan(None, None) == 4:
        label = "gemm_tn_dma_kernel" + label[len("gemm_tn_b16_kernel"):]      # the LDS-DMA kernel, not the register-staged one
    _profiler.records.append((label, flops, nbytes, e0, e1))


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().ispk_last_error_string()
        raise IspkError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def _dev(*tensors: Optional[Tensor]) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise IspkError("isp_tts_amd kernels need GPU tensors (got a CPU tensor); there is no CPU fallback")


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def device_info() -> tuple[str, int]:
    buf = ctypes.create_string_buffer(256)
    n = lib().ispk_device_info(buf, 256)
    if n <= 0:
        _check(n if n != 0 else -1, "ispk_device_info")
    return buf.value.decode(), n


def _rows2d(t: Tensor) -> Tensor:
    """[..., D] -> [rows, D] view with unit inner stride (copies only when the layout requires it)."""
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t.reshape(-1, t.shape[-1])


def _mask1d(mask: Optional[Tensor]) -> Optional[Tensor]:     # a row mask of any shape, flat and contiguous
    return None if mask is None else mask.reshape(-1).contiguous()


def _i64(t: Optional[Tensor]) -> Optional[Tensor]:           # lengths / ids as the kernels read them
    return None if t is None else t.to(torch.int64).contiguous()


def _ld(t: Optional[Tensor]) -> int:                         # leading stride of an optional operand
    return 0 if t is None else t.stride(0)


stage_calls = 0     # how many staging passes have been launched (train/graph.py checks that a capture recorded one)

# The wrappers, one module per kernel family.  Each reaches this core, and any wrapper, as `_rt.<name>` at call time, so a
# replaced `runtime._launch` or `runtime.<wrapper>` is seen by all of them.
from .bindings.gemm import *       # noqa: E402,F401,F403
from .bindings.layers import *     # noqa: E402,F401,F403
from .bindings.adaptor import *    # noqa: E402,F401,F403
from .bindings.util import *       # noqa: E402,F401,F403
from .bindings.train import *      # noqa: E402,F401,F403
from .bindings.evaluate import *   # noqa: E402,F401,F403
from .bindings.audio import *      # noqa: E402,F401,F403
from .bindings.vocoders import *   # noqa: E402,F401,F403
