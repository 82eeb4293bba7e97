"""ispk_attn_block_short_bf16 (csrc/attn_block.hip) against the three entry points it replaces, called in sequence through the C ABI:
ispk_gemm_bf16 (ISPK_EP_OUT_BF16: the q/kv rows), ispk_alibi_mqa_attn_bf16, ispk_gemm_bf16 (ISPK_EP_MASK_ACC + residual).

Cases: B = 3; N in {1, 32, 33, 64, 65, 100, 128} (one and two query tiles, on and +-1 around the 32-key blocks); key_len ragged
(N, 1, N // 2 + 1); both head / dim pairs (6 x 64 = 384, 4 x 64 = 256); both input forms (normalised rows: the kernel projects and
stores q/kv; finished q/kv rows).  Every case asserts
  * equality: the q/kv rows it stores and its fp32 output are torch.equal to the three launches' (every row, rows >= key_len too);
  * float64: the output against the block evaluated in float64 from the bf16 operands, within the bound tests/test_gpu_attention.py
    uses for the bf16 attention entry, 1.5e-2 * max(1, max |v| / 4) - weights are scaled by 1 / sqrt(dim), so q, k, v, the attention
    output and its projection are all O(1) like that test's operands;
  * rows >= key_len (mask = 0) of the output hold the residual's bits;
  * no stray stores and no reads outside the views: every operand and output is a view into a buffer filled with NaN bit patterns
    (8 padding elements per row, 3 rows after row B N, slack behind), everything outside an output view keeps those bits, and an
    input read from outside its view would show up as NaN in the output;
  * a second call writes the same bits.
Rows >= key_len INSIDE the views hold finite values, as in the model (LayerNorm of finite rows): the attention kernels mask a
key past key_len by zeroing its probability, and 0 x NaN in the P V product would still be NaN - for the three launches as well.
"""
import ctypes
import zlib

import pytest
import torch

from isp_tts_amd import runtime, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN32, NAN16 = 0x7FC0_1234, 0x7FC1
B = 3
NS = (1, 32, 33, 64, 65, 100, 128)
EP_OUT_BF16, EP_MASK_ACC = runtime.EP_OUT_BF16, runtime.EP_MASK_ACC


class Buf:
    """rows x (cols + 8) elements inside a NaN-filled backing buffer with 3 extra rows and slack behind."""

    def __init__(self, rows, cols, dt, fill=None):
        self.rows, self.cols, self.ld, self.dt = rows, cols, cols + 8, dt
        self.ib, self.nan = (torch.int32, NAN32) if dt == torch.float32 else (torch.int16, NAN16)
        self.back = torch.empty(((rows + 3) * self.ld + 256,), dtype=dt, device=DEV)
        self.back.view(self.ib).fill_(self.nan)
        self.mat = self.back[:rows * self.ld].view(rows, self.ld)
        if fill is not None:
            self.mat[:, :cols] = fill.reshape(rows, cols).to(dt)

    @property
    def view(self):
        return self.mat[:, :self.cols]

    def ptr(self):
        return self.mat.data_ptr()

    def bits(self):
        return self.back.view(self.ib).clone()

    def assert_outside_untouched(self, what):
        inside = torch.zeros(self.back.numel(), dtype=torch.bool, device=DEV)
        inside[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = True
        bad = (self.back.view(self.ib)[~inside] != self.nan).sum().item()
        assert bad == 0, f"{what}: {bad} elements outside the view were written"


def _rc(rc, what):
    if rc != 0:
        msg = runtime.lib().ispk_last_error_string()
        raise AssertionError(f"{what} refused (rc={rc}): {msg.decode() if msg else '?'}")


def _operands(H, N):
    """x, [Wq; Wkv], Wo (bf16), residual (fp32), slopes, key_len, row mask."""
    D = 64 * H
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(f"attn_block/{H}/{N}".encode()))
    x = torch.randn((B, N, D), generator=g, device=DEV).to(torch.bfloat16)
    wqkv = (torch.randn((D + 128, D), generator=g, device=DEV) / D ** 0.5).to(torch.bfloat16)
    wo = (torch.randn((D, D), generator=g, device=DEV) / D ** 0.5).to(torch.bfloat16)
    resid = torch.randn((B, N, D), generator=g, device=DEV)
    slopes = (torch.tensor(synth.alibi_default_slopes(H), device=DEV) * 1.1).float()
    key_len = torch.tensor([N, 1, N // 2 + 1], dtype=torch.int64, device=DEV)
    mask = (torch.arange(N, device=DEV)[None, :] < key_len[:, None]).to(torch.uint8)
    return x, wqkv, wo, resid, slopes, key_len, mask


def _three_launches(H, N, xb, qkvb, wqkv, wo, residb, slopes, key_len, mask, project):
    """-> out Buf; qkvb is written first when `project`."""
    L, st, D, R = runtime.lib(), runtime._stream(), 64 * H, B * N
    if project:
        _rc(L.ispk_gemm_bf16(xb.ptr(), xb.ld, wqkv.data_ptr(), D, qkvb.ptr(), qkvb.ld, None, None, 0, None, R, D + 128, D,
                             EP_OUT_BF16, 0, 0, st), "q/kv gemm")
    ob = Buf(R, D, torch.bfloat16)
    es = 2
    _rc(L.ispk_alibi_mqa_attn_bf16(qkvb.ptr(), qkvb.ld, qkvb.ptr() + D * es, qkvb.ptr() + (D + 64) * es, qkvb.ld, slopes.data_ptr(),
                                   key_len.data_ptr(), ob.ptr(), ob.ld, B, N, H, st), "attention")
    out = Buf(R, D, torch.float32)
    _rc(L.ispk_gemm_bf16(ob.ptr(), ob.ld, wo.data_ptr(), D, out.ptr(), out.ld, None, residb.ptr(), residb.ld, mask.data_ptr(), R, D,
                         D, EP_MASK_ACC, 0, 0, st), "to_out gemm")
    return out


def _fused(H, N, xb, qkvb, wqkv_c, wo_c, residb, slopes, key_len, mask, out):
    L, st = runtime.lib(), runtime._stream()
    _rc(L.ispk_attn_block_short_bf16(None if xb is None else xb.ptr(), 0 if xb is None else xb.ld,
                                     None if xb is None else wqkv_c.data_ptr(), qkvb.ptr(), qkvb.ld, slopes.data_ptr(),
                                     key_len.data_ptr(), wo_c.data_ptr(), residb.ptr(), residb.ld, mask.data_ptr(), out.ptr(), out.ld,
                                     B, N, H, st), "attn_block")


def _float64(H, N, qkv, wo, resid, slopes, key_len, mask):
    """The block from q/kv rows (float64 [B, N, D + 128]) on -> (out [B, N, D], max |v|)."""
    D = 64 * H
    q, k, v = qkv[..., :D].view(B, N, H, 64), qkv[..., D:D + 64], qkv[..., D + 64:]
    idx = torch.arange(N, device=DEV)
    s = torch.einsum("bihd,bjd->bhij", q, k) / 8.0 - slopes.double()[None, :, None, None] * (idx[:, None] - idx[None, :]).abs().double()
    s = s.masked_fill(idx[None, None, None, :] >= key_len.clamp(1, N)[:, None, None, None], float("-inf"))
    o = torch.einsum("bhij,bjd->bihd", torch.softmax(s, -1), v).reshape(B, N, D)
    return resid.double() + mask.double()[..., None] * (o @ wo.double().T), v.abs().max().item()


@pytest.mark.parametrize("form", ("rows", "qkv"))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("H", (6, 4))
def test_block_equals_the_three_launches(H, N, form):
    D, R = 64 * H, B * N
    x, wqkv, wo, resid, slopes, key_len, mask = _operands(H, N)
    project = form == "rows"
    xb, residb = Buf(R, D, torch.bfloat16, x), Buf(R, D, torch.float32, resid)
    qkv_ref = Buf(R, D + 128, torch.bfloat16)
    if not project:   # finished rows: the q/kv GEMM's, handed to both paths
        _rc(runtime.lib().ispk_gemm_bf16(xb.ptr(), xb.ld, wqkv.data_ptr(), D, qkv_ref.ptr(), qkv_ref.ld, None, None, 0, None, R, D + 128,
                                         D, EP_OUT_BF16, 0, 0, runtime._stream()), "q/kv gemm")
    out_ref = _three_launches(H, N, xb, qkv_ref, wqkv, wo, residb, slopes, key_len, mask, project)
    wqkv_c, wo_c = runtime.chunk_k16(wqkv), runtime.chunk_k16(wo)
    out = Buf(R, D, torch.float32)
    if project:
        qkvb = Buf(R, D + 128, torch.bfloat16)
    else:
        qkvb = Buf(R, D + 128, torch.bfloat16, qkv_ref.view)
    qkv_before = qkvb.bits()
    _fused(H, N, xb if project else None, qkvb, wqkv_c, wo_c, residb, slopes, key_len, mask, out)
    first = out.bits()

    # equality with the three launches
    if project:
        assert torch.equal(qkvb.view.view(torch.int16), qkv_ref.view.view(torch.int16)), "q/kv rows differ"
        qkvb.assert_outside_untouched("qkv")
    else:
        assert torch.equal(qkvb.bits(), qkv_before), "finished q/kv rows were written"
    diff = (out.view - out_ref.view).abs().nan_to_num(1e9).max().item()
    print(f"\nH={H} N={N} {form}: max |fused - three launches| = {diff:.3e}", end="")
    assert torch.equal(out.view.view(torch.int32), out_ref.view.view(torch.int32)), f"output differs: max |diff| {diff:.3e}"
    out.assert_outside_untouched("out")

    # float64
    qkv64 = x.double() @ wqkv.double().T if project else qkv_ref.view.reshape(B, N, D + 128).double()
    want, vmax = _float64(H, N, qkv64.reshape(B, N, D + 128), wo, resid, slopes, key_len, mask)
    err = (out.view.reshape(B, N, D).double() - want).abs().nan_to_num(1e9).max().item()
    err3 = (out_ref.view.reshape(B, N, D).double() - want).abs().nan_to_num(1e9).max().item()
    tol = 1.5e-2 * max(1.0, vmax / 4.0)
    print(f"  float64: {err:.3e} (three launches {err3:.3e}, tol {tol:.3e})", end="")
    assert err < tol, f"max |diff| to float64 {err:.3e} (tol {tol:.3e})"

    # rows >= key_len: the residual's bits
    pad = (mask == 0).reshape(R)
    assert torch.equal(out.view[pad].view(torch.int32), residb.view[pad].view(torch.int32)), "a masked row differs from the residual"

    _fused(H, N, xb if project else None, qkvb, wqkv_c, wo_c, residb, slopes, key_len, mask, out)
    assert torch.equal(out.bits(), first), "a second call wrote different bits"


def test_block_without_mask_and_key_len():
    """mask = NULL (every row valid) and key_len = NULL (= N): the plain residual epilogue."""
    H, N = 6, 100
    x, wqkv, wo, resid, slopes, _, _ = _operands(H, N)
    qkv = runtime.gemm(x, wqkv)
    o = runtime.alibi_mqa_attention(qkv, H, slopes, None)
    want = runtime.gemm(o, wo, resid=resid, out_dtype=torch.float32)
    got, qkv2 = runtime.attn_block_short(x, runtime.chunk_k16(wqkv), None, H, slopes, None, runtime.chunk_k16(wo), resid, None)
    assert torch.equal(qkv2, qkv) and torch.equal(got, want)
    got, _ = runtime.attn_block_short(None, None, qkv, H, slopes, None, runtime.chunk_k16(wo), resid, None)
    assert torch.equal(got, want)


def test_block_refuses_bad_arguments():
    L = runtime.lib()
    E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)   # never dereferenced: the checks run before any launch

    def call(x=one, ldx=384, wqkv=one, qkv=one, ld_qkv=512, slopes=one, wo=one, resid=one, ldr=384, out=one, ldo=384, Bn=2, N=100, H=6):
        return L.ispk_attn_block_short_bf16(x, ldx, wqkv, qkv, ld_qkv, slopes, None, wo, resid, ldr, None, out, ldo, Bn, N, H, None)

    assert call(qkv=None) == E_NULL and b"null" in L.ispk_last_error_string()
    assert call(wqkv=None) == E_NULL            # rows given without the projection weight
    assert call(resid=None) == E_NULL and call(out=None) == E_NULL and call(slopes=None) == E_NULL and call(wo=None) == E_NULL
    assert call(H=5) == E_UNSUP and call(H=8) == E_UNSUP
    assert call(N=129) == E_SHAPE and b"128" in L.ispk_last_error_string()
    assert call(N=0) == E_SHAPE and call(Bn=-1) == E_SHAPE and call(Bn=65536, N=1) == E_SHAPE
    assert call(ldx=256) == E_SHAPE and call(ld_qkv=384) == E_SHAPE and call(ldr=380) == E_SHAPE and call(ldo=128) == E_SHAPE
    assert call(ldx=388) == E_ALIGN and call(ld_qkv=516) == E_ALIGN and call(ldr=386) == E_ALIGN and call(ldo=390) == E_ALIGN
    assert call(x=odd) == E_ALIGN and call(qkv=odd) == E_ALIGN and call(out=odd) == E_ALIGN and call(resid=odd) == E_ALIGN
    assert call(Bn=0) == 0                       # an empty batch is a no-op
    assert call(x=None, wqkv=None, ldx=0, Bn=0) == 0
