"""Argument checks of the eight-wave feed-forward entry points (csrc/ffn2.hip), without a GPU.

Every case breaks exactly one condition of an otherwise valid call.  Pointers are `c_void_p(16)`, never dereferenced: the
checks come first, and `rows == 0` returns before any launch.  The expected codes pin what each entry point answers,
including where they differ from one another (minimum `inner`, NULL against UNSUPPORTED for a mask flag without a mask).
"""
import ctypes

import pytest

from isp_tts_amd import runtime

E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4
GELU, MASK_ACC, MASK_OUT = 1, 4, 8
P = ctypes.c_void_p(16)


def _proj(**tail):      # the arguments the projection entries share, up to `flags`
    return dict(x=P, ldx=384, attn_out=P, ld_attn=384, Wo=P, gamma=P, beta=P, eps=1e-5, W1=P, W2c=P, mask=None, out=P, ldo=384,
                rows=0, dim=384, inner=1536, flags=0, **tail)


# entry point -> (the short name its messages carry, a valid call in the order of the C signature)
ENTRIES = {
    "ispk_ffn_bf16_prenorm2": (b"ffn_prenorm2:", dict(
        x=P, ldx=384, gamma=P, beta=P, eps=1e-5, W1=P, W2c=P, mask=None, out=P, ldo=384, rows=0, dim=384, inner=1536, flags=0,
        row_stats=None, stats_eps=1e-5, stream=None)),
    "ispk_ffn_bf16_prenorm2_split": (b"ffn_prenorm2_split:", dict(
        x=P, ldx=384, gamma=P, beta=P, eps=1e-5, W1=P, W2c=P, parts=P, part_stride=128 * 384, splits=4, rows=0, dim=384,
        inner=1536, stream=None)),
    "ispk_attn_out_ffn_bf16": (b"attn_out_ffn:", _proj(row_stats=None, stats_eps=1e-5, stream=None)),
    # (the checks it shares with ispk_attn_out_ffn_bf16 speak as "attn_out_ffn", its own as "attn_out_ffn_qkv")
    "ispk_attn_out_ffn_qkv_bf16": (b"attn_out_ffn", _proj(next_gamma=P, next_beta=P, next_eps=1e-5, Wqkv=P, qkv=P, ld_qkv=512,
                                                          stream=None)),
    "ispk_attn_out_ffn_norm_bf16": (b"attn_out_ffn_norm:", _proj(final_gamma=P, final_beta=P, final_eps=1e-5, ln_mask=0, ln_out=P,
                                                                 ld_ln=384, ln_bf16=0, stream=None)),
    "ispk_attn_out_ffn_split_bf16": (b"attn_out_ffn_split:", dict(
        x=P, ldx=384, attn_out=P, ld_attn=384, Wo=P, gamma=P, beta=P, eps=1e-5, W1=P, W2c=P, mask=None, flags=0, parts=P,
        part_stride=128 * 384, splits=4, rows=0, dim=384, inner=1536, stream=None)),
}
EVERY = [(dict(), 0), (dict(x=None), E_NULL), (dict(dim=256), E_UNSUP), (dict(x=ctypes.c_void_p(8)), E_ALIGN),
         (dict(ldx=386), E_ALIGN)]
SPLIT_SHAPES = [(dict(inner=1536, splits=5), E_SHAPE), (dict(inner=64, splits=2), E_SHAPE),
                (dict(rows=128, part_stride=384), E_SHAPE)]
CASES = {
    "ispk_ffn_bf16_prenorm2": [
        (dict(inner=48), E_SHAPE), (dict(inner=32), 0), (dict(flags=GELU), E_UNSUP), (dict(flags=MASK_OUT), E_NULL),
        (dict(ldo=380), E_ALIGN), (dict(row_stats=ctypes.c_void_p(4)), E_ALIGN)],
    "ispk_attn_out_ffn_bf16": [(dict(attn_out=None), E_NULL), (dict(inner=32), E_SHAPE), (dict(ld_attn=388), E_ALIGN)],
    "ispk_attn_out_ffn_qkv_bf16": [(dict(next_gamma=None), E_NULL), (dict(ld_qkv=504), E_ALIGN)],
    "ispk_attn_out_ffn_norm_bf16": [
        (dict(ln_out=None), E_NULL), (dict(ln_mask=1), E_NULL), (dict(out=None), 0), (dict(ld_ln=380), E_ALIGN),
        (dict(ln_out=ctypes.c_void_p(8), ln_bf16=0), E_ALIGN), (dict(ln_out=ctypes.c_void_p(8), ln_bf16=1), 0)],
    "ispk_ffn_bf16_prenorm2_split": SPLIT_SHAPES,
    "ispk_attn_out_ffn_split_bf16": SPLIT_SHAPES + [(dict(flags=MASK_OUT), E_UNSUP), (dict(flags=MASK_ACC), E_UNSUP)],
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_argument_checks(entry):
    lib = runtime.lib()
    name, valid = ENTRIES[entry]
    for change, want in EVERY + CASES[entry]:
        assert set(change) <= set(valid), change
        got = getattr(lib, entry)(*{**valid, **change}.values())
        assert got == want, f"{entry}{change}: {got}, expected {want} ({lib.ispk_last_error_string()!r})"
        if want != 0:
            assert name in lib.ispk_last_error_string(), f"{entry}{change}: {lib.ispk_last_error_string()!r}"
