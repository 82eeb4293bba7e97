"""CPU: the C-ABI library builds, loads, exports every symbol include/ispk.h declares, and validates arguments
without touching a GPU (argument checks run before any launch)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from isp_tts_amd import runtime


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "ispk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ispk_[a-z0-9_]+)\s*\(", src)))


def test_build_entry_point_runs():
    import __graft_entry__
    __graft_entry__.build()
    assert os.path.exists(runtime.LIB_PATH)
    assert os.path.exists(os.path.join(ROOT, "oracle", "_build", "libmas_oracle.so"))


def test_every_header_symbol_is_exported_and_bound():
    syms = _header_symbols()
    assert len(syms) >= 12
    assert syms == sorted(runtime.SIGNATURES), "runtime.SIGNATURES must list exactly the header's entry points"
    handle = ctypes.CDLL(runtime.LIB_PATH)
    for s in syms:
        assert hasattr(handle, s), f"{s} is declared in include/ispk.h but missing from libispk.so"
    assert runtime.lib().ispk_abi_version() == 2


def test_signatures_come_from_the_header():
    """runtime reads argtypes, restypes and the ABI version from include/ispk.h.  Known answers: rows of the table that
    the runtime module used to keep by hand, which together use every C type the header does."""
    P, I32, I64, U32, U64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
    F32, F64 = ctypes.c_float, ctypes.c_double
    known = {
        "ispk_mas_f32": [P, P, P, P, P, P, I32, I32, I32, I64, I64, P],
        "ispk_device_info": [ctypes.c_char_p, I32],
        "ispk_gemm_f32": [P, I64, P, I64, P, I64, P, P, I64, P, I32, I32, I32, U32, I32, I64, P],
        "ispk_gemm_bf16_gelu_train": [P, I64, P, I64, P, I64, P, I64, I32, I32, I32, F32, U64, P],
        "ispk_audio_measure_f64": [P, I64, P, P, I64, P, P, P, P, P, I64, I32, I32, I32, I32, F64, I32, I32, F64, F64, P],
        "ispk_abi_version": [],
    }
    for name, argtypes in known.items():
        assert runtime.SIGNATURES[name] == argtypes, name
    assert [n for n, r in runtime.RESTYPES.items() if r is ctypes.c_char_p] == ["ispk_last_error_string"]
    assert all(r is I32 for n, r in runtime.RESTYPES.items() if n != "ispk_last_error_string")
    assert runtime.ABI_VERSION == 2
    assert len(runtime.SIGNATURES) == len(runtime.RESTYPES) == len(_header_symbols())


def test_header_parser_is_strict():
    version = "#define ISPK_ABI_VERSION 7 /* a comment that begins behind a #define\n   int32_t ispk_hidden(void); and ends here */\n"
    text = version + "int32_t ispk_y(const float* x, /* rows\n of */ int64_t ldx,\n    ispk_stream_t stream);\nconst char *ispk_z(void);"
    argtypes, restypes, abi = runtime._parse_header(text)
    assert argtypes == {"ispk_y": [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p], "ispk_z": []}
    assert restypes == {"ispk_y": ctypes.c_int32, "ispk_z": ctypes.c_char_p} and abi == 7
    # only the non-const char* is a string buffer; any other pointer is an address
    assert runtime._parse_header(version + "int32_t ispk_x(const char* s, char* d);")[0] == {"ispk_x": [ctypes.c_void_p, ctypes.c_char_p]}
    for bad in ("int32_t ispk_x(size_t n);",            # a type the map does not know
                "int32_t ispk_x(int32_t);",             # no parameter name to tell from a type
                "int32_t ispk_x(float v[4]);",
                "int32_t ispk_x(unsigned n);",
                "void ispk_x(void);",
                "int32_t ispk_x(void (*f)(int));",
                "int32_t ispk_x(void); int32_t ispk_x(void);"):
        with pytest.raises(runtime.IspkError, match="ispk_x"):
            runtime._parse_header(version + bad)
    with pytest.raises(runtime.IspkError, match="ISPK_ABI_VERSION"):
        runtime._parse_header("int32_t ispk_x(void);")


def test_missing_header_is_an_error(tmp_path):
    """The runtime module run from a tree without include/ispk.h (its own IspkError class: the module body runs in a scratch scope)."""
    scope = {"__name__": "isp_tts_amd.runtime", "__package__": "isp_tts_amd", "__file__": str(tmp_path / "isp_tts_amd" / os.path.basename(runtime.__file__))}
    with pytest.raises(RuntimeError, match=r"ispk\.h cannot be read") as e:
        exec(compile(open(runtime.__file__).read(), runtime.__file__, "exec"), scope)
    assert type(e.value).__name__ == "IspkError" and str(tmp_path) in str(e.value)


def test_runtime_names_resolve():
    """Every `runtime.<name>` that a Python file of the tree spells exists: the tools are run by no other test."""
    skip = {"_ref", "_build", "build", "__pycache__"}      # build products and compiled reference binaries
    files, missing = 0, []
    for base, dirs, names in os.walk(ROOT):
        dirs[:] = [d for d in dirs if not d.startswith(".") and d not in skip]
        for f in names:
            path = os.path.join(base, f)
            if not f.endswith(".py") or os.path.samefile(path, runtime.__file__):
                continue
            text = open(path).read()
            if not re.search(r"^\s*(from\s+[\w.]+\s+)?import\s+.*\bruntime\b", text, flags=re.M):
                continue
            files += 1
            missing += [(os.path.relpath(path, ROOT), n) for n in set(re.findall(r"(?<![\w.])runtime\.([A-Za-z_]\w*)", text))
                        if not hasattr(runtime, n)]
    assert files >= 70 and not missing, missing


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4
    assert lib.ispk_mas_f32(None, None, None, None, None, None, 1, 8, 8, 64, 8, None) == E_NULL
    assert b"null" in lib.ispk_last_error_string()
    one = ctypes.c_void_p(16)  # never dereferenced: shape checks fail first
    assert lib.ispk_mas_f32(one, one, one, one, None, None, 1, 8, 513, 8 * 513, 513, None) == E_SHAPE
    assert b"512" in lib.ispk_last_error_string()
    assert lib.ispk_mas_f32(one, one, one, one, None, None, 1, 4096, 512, 4096 * 512, 512, None) == E_SHAPE
    assert b"LDS" in lib.ispk_last_error_string()
    assert lib.ispk_gemm_f32(one, 12, one, 12, one, 8, None, None, 0, None, 4, 8, 12, 0, 0, 0, None) == E_SHAPE
    assert lib.ispk_gemm_f32(one, 18, one, 16, one, 8, None, None, 0, None, 4, 8, 16, 0, 0, 0, None) == E_ALIGN
    assert lib.ispk_gemm_f32(one, 16, one, 16, one, 8, None, None, 0, None, 4, 8, 16, 4, 0, 0, None) == E_NULL  # mask flag
    assert lib.ispk_gemm_f32(one, 16, one, 16, one, 8, None, None, 0, None, 4, 8, 16, 64, 0, 0, None) == E_UNSUP
    assert lib.ispk_layernorm_f32(one, 100, None, None, None, None, 0, 1, None, one, 100, 4, 100, 1e-5, None) == E_SHAPE
    assert lib.ispk_alibi_mqa_attn_f32(one, 384, one, one, 128, one, None, one, 384, 2, 16, 9, None) == E_SHAPE
    assert lib.ispk_alibi_mqa_attn_f32(one, 384, one, one, 126, one, None, one, 384, 2, 16, 6, None) == E_ALIGN
    assert lib.ispk_linear_small_f32(None, 1, None, 1, None, None, 0, None, 1, 1, 1, 1, 0, None) == E_NULL
    assert lib.ispk_gemm_f32_tile(32768, 384, 384) == 22 and lib.ispk_gemm_f32_tile(6400, 384, 384) == 12


def test_zero_sized_batches_are_noops():
    lib = runtime.lib()
    one = ctypes.c_void_p(16)
    assert lib.ispk_mas_f32(one, one, one, one, None, None, 0, 8, 8, 64, 8, None) == 0
    assert lib.ispk_gemm_f32(one, 16, one, 16, one, 8, None, None, 0, None, 0, 8, 16, 0, 0, 0, None) == 0
    assert lib.ispk_layernorm_f32(one, 64, None, None, None, None, 0, 1, None, one, 64, 0, 64, 1e-5, None) == 0


def test_product_fails_loudly_without_gpu_or_library(monkeypatch, tmp_path):
    import torch
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.gemm(torch.zeros(8, 64), torch.zeros(16, 64))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.mas(torch.zeros(1, 4, 4), torch.tensor([4]), torch.tensor([4]))
    monkeypatch.setattr(runtime, "_lib", None)
    monkeypatch.setattr(runtime, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(runtime.IspkError, match="not built"):
        runtime.lib()
