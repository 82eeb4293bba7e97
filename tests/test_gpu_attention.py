"""float64 matrix of the ALiBi-MQA attention entry points, called through the C ABI.

Entries: ispk_alibi_mqa_attn_f32, _bf16 / _bf16_tiles, _split_f16 (fp32 output), the fp32 training pair
(ispk_alibi_mqa_attn_train_f32 / _bwd_f32) and the bf16 training pair (_train_bf16 / _bwd_bf16).

Reference (include/ispk.h): o[b][i][h] = sum_j softmax_j(q_ih . k_j / 8 - slope_h |i - j|) v_j over j < clamp(key_len[b], 1, N),
evaluated in float64 on the GPU from the operands the kernel saw (bf16-rounded for the bf16 entries, fp32 otherwise), for ALL
query rows (rows i >= key_len are defined).  With dropout the probabilities are multiplied by keep / (1 - p), keep exported by
ispk_dropout_mask_u8 at index ((b H + h) N + i) N + j.  Gradients are float64 autograd of the same formula; the backwards take
`o` as an input (delta_i = sum_d o_id dO_id), so the reference uses the o the kernel was given for delta too (see _ref_backward).

Every case also checks
  * no stray stores: each output lives in a buffer filled with a NaN sentinel (padding columns, an offset before the view, three
    rows after row B N, slack after the end); everything outside the view keeps the sentinel's bits.  Input padding is NaN, so
    a read outside an operand's view shows up as NaN output;
  * reproducibility: a second call writes the same bits into the whole backing buffer.
Layouts: (a) contiguous fused [Q|K|V]; (b) ldq = ld_qkv = row + 8, NaN padding; (c) separate Q and K/V buffers, ldkv != ldq,
V not adjacent to K (inference entries); (d) ldo / ld_o = H 64 + 8 with the output 4 elements past the buffer's start;
(de) the training pairs: forward as (d), backward with o / d_o at ld_o = H 64 + 8, ld_qkv = row + 8 and dqkv 4 elements in.

The dispatch is a pure function of (B, N, H, qpw); each case id names the kernel instance and branch it reaches."""
import zlib
from dataclasses import dataclass
from typing import Optional

import pytest
import torch

from isp_tts_amd import runtime, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLACK = 256
NAN32 = 0x7FC0_1234            # sentinel bit patterns (quiet NaNs with payloads no kernel produces)
NAN16 = 0x7FC1
NS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 640, 1025, 1723)   # 1723: the recipes' data bound
PATTERNS = ("null", "full", "one", "zero", "over", "ragged")
EDGES_LO = (31, 32, 33, 63, 64, 65, 127, 128, 129)         # on and +-1 around the 32-, 64- and 128-key block edges
EDGES_HI = (511, 512, 513, 127, 128, 129, 1, 0, 2000)      # ... the 512-key ring / staging boundary, mixed with 1, 0, > N
SEED = 4242


# ------------------------------------------------------------------------------------------------------- dispatch mirror
def _bf16_plan(B, N, H, qpw):
    """(MAXT, IPL, effective qpw) of ispk_alibi_mqa_attn_bf16_tiles (csrc/attention.hip)."""
    nqt = (N + 63) // 64
    eff = 1
    if N <= 512:
        while eff < 4 and B * ((nqt + 2 * eff - 1) // (2 * eff)) >= 256:
            eff *= 2
    if qpw > 0:
        eff = qpw if N <= 512 else 1
    maxt, ipl = (1024, 4) if H >= 7 else (768, 4) if H >= 4 else (768, 8) if H >= 2 else (768, 16)
    return maxt, ipl, eff


def _branch(entry, B, N, H, qpw):
    if entry == "f32":
        return "attn_f32_kernel" + ("<384,16>" if H <= 3 else "<768>" if H <= 6 else "<1024>")
    if entry == "bf16":
        maxt, ipl, eff = _bf16_plan(B, N, H, qpw)
        ring = "resident" if N <= 512 else "streamed"
        return f"attn_bf16_kernel<{maxt},{ipl}>-{ring}-qpw{eff}" + ("auto" if qpw == 0 else f"of{qpw}")
    if entry == "split":
        return {5: "split-4+1", 7: "split-6+1", 8: "split-6+2"}.get(H, "split-one")
    if entry == "train_f32":
        return "train_f32-32row"
    return f"train_bf16-64row-{(N + 511) // 512}round"


@dataclass(frozen=True)
class Case:
    entry: str
    B: int
    N: int
    H: int
    lens: Optional[tuple]
    layout: str
    family: str = "normal"       # normal | spike_more | spike_less | big_slope
    qpw: int = 0                 # bf16 forward: 0 automatic, else forced
    p: float = 0.0               # training pairs: dropout
    lse_in: bool = True          # fp32 backward: take the forward's lse (else recompute)
    dopad: bool = False          # backward: d_o left non-zero on padded query rows

    @property
    def id(self):
        kl = "null" if self.lens is None else "kl" + ".".join(str(x) for x in self.lens[:9])
        s = f"{self.entry}-{_branch(self.entry, self.B, self.N, self.H, self.qpw)}-B{self.B}N{self.N}H{self.H}-{kl}-L{self.layout}"
        if self.family != "normal":
            s += "-" + self.family
        if self.entry.startswith("train"):
            s += f"-p{self.p:g}" + ("" if self.entry == "train_bf16" or self.lse_in else "-recompute") + ("-dopad" if self.dopad else "")
        return s


def _lens(pattern, N, B):
    if pattern == "null":
        return None
    if pattern == "full":
        return (N,) * B
    if pattern == "one":
        return (1,) * B
    if pattern == "zero":
        return (0,) * B
    if pattern == "over":
        return (N + 1, N + 1000)[:B]
    return (N, 1, 0, N + 7, 33, 64, 129, 511, 513)[:B]     # ragged: mixes the above with block edges


def _cases():
    cases = []
    ent_h = {"f32": range(1, 9), "bf16": range(1, 9), "split": range(1, 9), "train_f32": range(1, 9),
             "train_bf16": range(1, 7)}
    lay = {"f32": "abcd", "bf16": "abcd", "split": "abcd", "train_f32": ("a", "b", "de"), "train_bf16": ("a", "b", "de")}
    for e, hs in ent_h.items():
        hs = list(hs)
        train = e.startswith("train")
        for n_i, N in enumerate(NS):
            pat = PATTERNS[n_i % len(PATTERNS)]
            B = 5 if pat == "ragged" else 2
            kw = dict(p=(0.0, 0.1)[n_i % 2], lse_in=n_i % 4 < 2) if train else {}
            cases.append(Case(e, B, N, hs[n_i % len(hs)], _lens(pat, N, B), lay[e][n_i % len(lay[e])], **kw))
        # key lengths on and around the block edges (B = 9), the 512-key boundary, value families
        tkw = (lambda **k: k) if train else (lambda **k: {})
        cases.append(Case(e, 9, 640, hs[-1], EDGES_LO, lay[e][1], **tkw(p=0.1, lse_in=True)))
        cases.append(Case(e, 9, 1025, hs[len(hs) // 2], EDGES_HI, lay[e][-1], **tkw(p=0.0, lse_in=False)))
        cases.append(Case(e, 3, 700, hs[1], (700, 700, 650), lay[e][0], "spike_more", **tkw(p=0.0)))
        cases.append(Case(e, 2, 300, hs[-2], None, lay[e][-1], "spike_less", **tkw(p=0.1)))
        cases.append(Case(e, 2, 1723, hs[2], (1723, 900), lay[e][1], "big_slope", **tkw(p=0.0, lse_in=False)))
        if train:
            cases.append(Case(e, 2, 160, hs[3], (160, 97), lay[e][-1], p=0.3))
            cases.append(Case(e, 3, 200, hs[4], (200, 150, 33), lay[e][0], p=0.1, dopad=True))
            cases.append(Case(e, 3, 200, hs[4], (200, 150, 33), lay[e][1], p=0.0, dopad=True, lse_in=False))
    # bf16 forward: forced query tiles per workgroup (tile counts that qpw does not divide, qpw > tile count, N > 512 where
    # a forced value falls back to 1) and batches large enough for the launcher to pick qpw > 1 by itself
    for qpw, N, H, layout in ((1, 300, 6, "a"), (2, 300, 3, "b"), (3, 300, 8, "c"), (4, 300, 1, "d"), (3, 511, 5, "a"),
                              (8, 200, 2, "b"), (8, 512, 4, "d"), (4, 640, 6, "c"), (2, 1723, 7, "a"), (3, 65, 3, "d")):
        cases.append(Case("bf16", 3, N, H, (N, max(N // 3, 1), N - 31), layout, qpw=qpw))
    cases.append(Case("bf16", 300, 33, 4, None, "a"))               # nqt = 1: automatic qpw 4 > tile count
    cases.append(Case("bf16", 260, 511, 6, tuple((7 * i) % 530 for i in range(260)), "d"))   # automatic qpw 4, ragged
    cases.append(Case("bf16", 256, 129, 2, None, "b", "spike_more"))            # automatic qpw 4 over 3 tiles
    return cases


CASES = _cases()


# ------------------------------------------------------------------------------------------------------- operands
def _operands(c: Case):
    """Logical operands as float64 on the GPU (already rounded to what the kernel sees) and the slopes."""
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(f"{c.entry}/{c.B}/{c.N}/{c.H}/{c.family}".encode()))
    B, N, H = c.B, c.N, c.H
    q = torch.randn((B, N, H, 64), generator=g, device=DEV)
    k = torch.randn((B, N, 64), generator=g, device=DEV)
    v = torch.randn((B, N, 64), generator=g, device=DEV)
    slopes = torch.tensor(synth.alibi_default_slopes(H), device=DEV) * 1.1
    if c.family.startswith("spike"):
        # a late key raises every query's running maximum: u . u / 8 = 8 per unit of `amp`, on top of scores ~ N(0, 1).
        # spike_more: + ~96 nats (138 exp2 units: far above kLazy = 16, and an un-rescaled exp2 would overflow fp32);
        # spike_less: + ~10 nats (~14 exp2 units above the scale of the earlier maxima: it must not).
        u = torch.where(torch.randn((64,), generator=g, device=DEV) > 0, 1.0, -1.0)
        amp = 12.0 if c.family == "spike_more" else 1.25
        q = q * 0.25 + u
        for j in sorted({N - 1, (3 * N) // 4, max(N - 130, 0)}):
            k[:, j] = amp * u
        slopes = torch.full((H,), 0.01, device=DEV)
    if c.family == "big_slope":     # the bias dominates: most weights underflow to 0
        slopes = torch.linspace(1.0, 0.3, H, device=DEV) if H > 1 else torch.ones(1, device=DEV)
    if c.entry in ("bf16", "train_bf16"):
        q, k, v = (t.to(torch.bfloat16).float() for t in (q, k, v))
    return q.double(), k.double(), v.double(), slopes.float()


def _klen(c: Case):
    """clamp(key_len, 1, N) per batch item (the contract of include/ispk.h)."""
    if c.lens is None:
        return torch.full((c.B,), c.N, dtype=torch.int64, device=DEV)
    return torch.tensor(c.lens, dtype=torch.int64, device=DEV).clamp(1, c.N)


def _keep(c: Case):
    if c.p == 0.0:
        return None
    return runtime.dropout_mask(c.B * c.H * c.N * c.N, c.p, SEED, DEV).view(c.B, c.H, c.N, c.N)


# ------------------------------------------------------------------------------------------------------- reference
def _scores(q, k, slopes, kl, b0, b1):
    N = q.shape[1]
    idx = torch.arange(N, device=DEV)
    dist = (idx[:, None] - idx[None, :]).abs().double()
    s = torch.einsum("bihd,bjd->bhij", q[b0:b1], k[b0:b1]) / 8.0 - slopes.double()[None, :, None, None] * dist
    return s.masked_fill(idx[None, None, None, :] >= kl[b0:b1, None, None, None], float("-inf"))


def _chunk(H, N):
    return max(1, (1 << 25) // (H * N * N))


def _ref_forward(q, k, v, slopes, kl, keep, p):
    """-> o [B, N, H, 64], lse [B, H, N], |row max| (the magnitude of the scores that carry the weight, for the bounds)."""
    B, N, H, _ = q.shape
    o = torch.empty_like(q)
    lse = torch.empty((B, H, N), dtype=torch.float64, device=DEV)
    mag = 0.0
    for b0 in range(0, B, _chunk(H, N)):
        b1 = min(B, b0 + _chunk(H, N))
        s = _scores(q, k, slopes, kl, b0, b1)
        mag = max(mag, s.amax(-1).abs().max().item())
        l = torch.logsumexp(s, -1)
        pr = torch.exp(s - l[..., None])
        if keep is not None:
            pr = pr * keep[b0:b1] / (1.0 - p)
        o[b0:b1] = torch.einsum("bhij,bjd->bihd", pr, v[b0:b1])
        lse[b0:b1] = l
    return o, lse, mag


def _ref_backward(q, k, v, slopes, kl, keep, p, o_given, d_o):
    """float64 autograd of the forward formula.  The kernels form delta_i = sum_d o_id dO_id from the o they are GIVEN (the
    forward's fp32 / bf16 output); exact autograd uses the exact o.  Adding (delta_exact - delta_given)_i lse_i (a constant
    times lse: its gradient is that constant times P_ij) to the loss turns autograd's dS = P (dP - delta_exact) into the
    kernels' P (dP - delta_given), and changes nothing else."""
    B, N, H, _ = q.shape
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    lsl = torch.log(slopes.double()).requires_grad_()
    for b0 in range(0, B, _chunk(H, N)):
        b1 = min(B, b0 + _chunk(H, N))
        qb, kb, vb = (t[b0:b1].clone().requires_grad_() for t in (q, k, v))
        idx = torch.arange(N, device=DEV)
        dist = (idx[:, None] - idx[None, :]).abs().double()
        s = torch.einsum("bihd,bjd->bhij", qb, kb) / 8.0 - lsl.exp()[None, :, None, None] * dist
        s = s.masked_fill(idx[None, None, None, :] >= kl[b0:b1, None, None, None], float("-inf"))
        lse = torch.logsumexp(s, -1)
        pr = torch.exp(s - lse[..., None])
        if keep is not None:
            pr = pr * keep[b0:b1] / (1.0 - p)
        o = torch.einsum("bhij,bjd->bihd", pr, vb)
        g = d_o[b0:b1]
        corr = ((o.detach() - o_given[b0:b1]) * g).sum(-1).transpose(1, 2)        # [b, H, N]
        ((o * g).sum() + (corr * lse).sum()).backward()
        dq[b0:b1], dk[b0:b1], dv[b0:b1] = qb.grad, kb.grad, vb.grad
    return dq, dk, dv, lsl.grad


# ------------------------------------------------------------------------------------------------------- buffers
def _bits(dt):
    return (torch.int32, NAN32) if dt == torch.float32 else (torch.int16, NAN16)


class Buf:
    """rows x ld elements at element offset `off` of a NaN-filled backing buffer with 3 extra rows and SLACK after."""

    def __init__(self, rows, ld, dt, off=0):
        self.rows, self.ld, self.dt, self.off = rows, ld, dt, off
        ib, nan = _bits(dt)
        self.back = torch.empty((off + (rows + 3) * ld + SLACK,), dtype=dt, device=DEV)
        self.back.view(ib).fill_(nan)
        self.mat = self.back[off:off + rows * ld].view(rows, ld)

    def ptr(self, col=0):
        return self.mat.data_ptr() + col * self.back.element_size()

    def snapshot(self):
        return self.back.view(_bits(self.dt)[0]).clone()

    def assert_outside_untouched(self, cols, what):
        """Everything but mat[:, :cols] still holds the sentinel's bits."""
        ib, nan = _bits(self.dt)
        inside = torch.zeros(self.back.numel(), dtype=torch.bool, device=DEV)
        inside[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :cols] = True
        bad = (self.back.view(ib)[~inside] != nan).sum().item()
        assert bad == 0, f"{what}: {bad} elements outside the output view were written"


def _put(buf: Buf, col, x):
    """x [rows, w] (float64) -> buf.mat[:, col:col+w] in the buffer's dtype."""
    buf.mat[:, col:col + x.shape[1]] = x.to(buf.dt)


def _out_buf(layout, rows, H, dt):
    return Buf(rows, H * 64 + 8, dt, 4) if layout in ("d", "de") else Buf(rows, H * 64, dt)


def _kl_tensor(c: Case):
    return None if c.lens is None else torch.tensor(c.lens, dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------- calls
def _rc(rc, what):
    if rc != 0:
        msg = runtime.lib().ispk_last_error_string()
        raise AssertionError(f"{what} refused (rc={rc}): {msg.decode() if msg else '?'}")


def _inference_inputs(c, q, k, v, dt):
    B, N, H = c.B, c.N, c.H
    rows, W = B * N, H * 64 + 128
    qr, kr, vr = q.reshape(rows, H * 64), k.reshape(rows, 64), v.reshape(rows, 64)
    if c.layout == "c":
        qb, kvb = Buf(rows, H * 64 + 24, dt), Buf(rows, 152, dt)
        _put(qb, 0, qr)
        _put(kvb, 0, kr)
        _put(kvb, 72, vr)
        return (qb, kvb), qb.ptr(), qb.ld, kvb.ptr(0), kvb.ptr(72), kvb.ld
    buf = Buf(rows, W + (8 if c.layout == "b" else 0), dt)
    _put(buf, 0, qr)
    _put(buf, H * 64, kr)
    _put(buf, H * 64 + 64, vr)
    return (buf,), buf.ptr(), buf.ld, buf.ptr(H * 64), buf.ptr(H * 64 + 64), buf.ld


def _call_inference(c, ins, out: Buf, slopes, kl, qpw=None):
    L, st = runtime.lib(), runtime._stream()
    _, qp, ldq, kp, vp, ldkv = ins
    kp_ = None if kl is None else kl.data_ptr()
    B, N, H = c.B, c.N, c.H
    if c.entry == "f32":
        rc = L.ispk_alibi_mqa_attn_f32(qp, ldq, kp, vp, ldkv, slopes.data_ptr(), kp_, out.ptr(), out.ld, B, N, H, st)
    elif c.entry == "bf16":
        q_t = c.qpw if qpw is None else qpw
        if q_t == 0:
            rc = L.ispk_alibi_mqa_attn_bf16(qp, ldq, kp, vp, ldkv, slopes.data_ptr(), kp_, out.ptr(), out.ld, B, N, H, st)
        else:
            rc = L.ispk_alibi_mqa_attn_bf16_tiles(qp, ldq, kp, vp, ldkv, slopes.data_ptr(), kp_, out.ptr(), out.ld, B, N, H,
                                                  q_t, st)
    else:
        rc = L.ispk_alibi_mqa_attn_split_f16(qp, ldq, kp, vp, ldkv, slopes.data_ptr(), kp_, out.ptr(), out.ld, 0, B, N, H, st)
    _rc(rc, c.entry)


# ------------------------------------------------------------------------------------------------------- tolerances
# Scores are formed in fp32 at the magnitude of the row's maximum |m| (ALiBi bias included: slope * distance reaches 1,700
# for big slopes on far padded rows), so a score carries an absolute error of a few 2^-24 |m| and each weight the same
# relative error: the bounds scale by max(1, |m| / 64) - the existing tests' regime has |m| < 64 and keeps its bound (as the
# fp32 inference test's own N / 256 factor, which this refines).  The split path's operands carry 22 significant bits, not 24:
# max(1, |m| / 16) (the existing split test's valid rows have |m| < 16).
def _scale(mag, bits=24):
    return max(1.0, mag / 2.0 ** (bits - 18))


def _err(got, want, mask=None):
    d = (got.double() - want).abs()
    if mask is not None:
        d = d * mask
    assert not torch.isnan(got).any(), "NaN in the output view"
    return d.max().item()


# ------------------------------------------------------------------------------------------------------- the matrix
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """After the module: the worst error of each entry and output relative to its float64 scale (shown with -s)."""
    yield
    for (e, what), rel in sorted(WORST.items()):
        print(f"\nworst {e:10s} {what:9s} {rel:.3e}", end="")


def _record(entry, what, rel):
    WORST[(entry, what)] = max(WORST.get((entry, what), 0.0), rel)


def _run_inference(c):
    dt = torch.float32 if c.entry in ("f32", "split") else torch.bfloat16
    q, k, v, slopes = _operands(c)
    kl = _kl_tensor(c)
    o_ref, _, mag = _ref_forward(q, k, v, slopes, _klen(c), None, 0.0)
    rows, H = c.B * c.N, c.H
    ins = _inference_inputs(c, q, k, v, dt)
    out = _out_buf(c.layout, rows, H, dt)
    _call_inference(c, ins, out, slopes, kl)
    first = out.snapshot()
    got = out.mat[:, :H * 64].reshape(c.B, c.N, H, 64)
    err = _err(got, o_ref)
    scale = o_ref.abs().max().item()
    _record(c.entry, "o", err / scale)
    if c.entry == "f32":
        # exact fp32 products: the existing bound of test_gpu_kernels.py, 2e-5 absolute (N / 256 for the bias)
        tol = 2e-5 * max(1.0, c.N / 256, mag / 64)
    elif c.entry == "bf16":
        # bf16 P (2^-9 relative per weight) and a bf16 output (2^-9 relative): 1.5e-2 absolute on O(1) outputs
        # (test_gpu_kernels.py), i.e. values |v| <= 4.  Both roundings are relative, so beyond that the bound scales with max |v|.
        tol = 1.5e-2 * max(1.0, v.abs().max().item() / 4.0)
    else:
        # split fp16 (22 bits) products, v_exp_f32: 1e-5 absolute (test_gpu_split.py), scaled with the score magnitude
        tol = 1e-5 * _scale(mag, 22)
    assert err < tol, f"o: max |diff| {err:.3e} (tol {tol:.3e}, scale {scale:.3e}, |m| {mag:.1f})"
    out.assert_outside_untouched(H * 64, "out")
    _call_inference(c, ins, out, slopes, kl)
    assert torch.equal(out.snapshot(), first), "a second call wrote different bits"
    if c.entry == "bf16" and c.qpw > 1:      # forced tiles per workgroup: identical bits to one tile per workgroup
        one = _out_buf(c.layout, rows, H, dt)
        _call_inference(c, ins, one, slopes, kl, qpw=1)
        assert torch.equal(one.snapshot(), first), "forced qpw changed the result"


def _call_train_fwd(c, qkvb: Buf, slopes, kl, o: Buf, lse: Buf):
    L = runtime.lib()
    fn = L.ispk_alibi_mqa_attn_train_f32 if c.entry == "train_f32" else L.ispk_alibi_mqa_attn_train_bf16
    _rc(fn(qkvb.ptr(), qkvb.ld, slopes.data_ptr(), None if kl is None else kl.data_ptr(), o.ptr(), o.ld, lse.ptr(), c.B, c.N,
           c.H, c.p, SEED, runtime._stream()), c.entry + " forward")


def _ws_floats(c):
    if c.entry == "train_f32":
        return 2 * c.B * c.H * c.N + c.H * c.B * ((c.N + 31) // 32)
    return c.B * c.H * c.N + 2 * c.H * c.B * ((c.N + 63) // 64)


def _call_train_bwd(c, qkvb, ob, dob, slopes, kl, lse, dq: Buf, dls: Buf, ws):
    L, st = runtime.lib(), runtime._stream()
    klp = None if kl is None else kl.data_ptr()
    if c.entry == "train_f32":
        rc = L.ispk_alibi_mqa_attn_bwd_f32(qkvb.ptr(), qkvb.ld, ob.ptr(), dob.ptr(), ob.ld, slopes.data_ptr(), klp, dq.ptr(),
                                           dls.ptr(), ws.data_ptr(), ws.numel(), c.B, c.N, c.H,
                                           lse.ptr() if c.lse_in else None, c.p, SEED, st)
    else:
        rc = L.ispk_alibi_mqa_attn_bwd_bf16(qkvb.ptr(), qkvb.ld, ob.ptr(), dob.ptr(), ob.ld, slopes.data_ptr(), klp, lse.ptr(),
                                            dq.ptr(), dls.ptr(), ws.data_ptr(), ws.numel(), c.B, c.N, c.H, c.p, SEED, st)
    _rc(rc, c.entry + " backward")


def _run_training(c):
    dt = torch.float32 if c.entry == "train_f32" else torch.bfloat16
    f32 = dt == torch.float32
    B, N, H = c.B, c.N, c.H
    rows, W = B * N, H * 64 + 128
    q, k, v, slopes = _operands(c)
    kl, klc = _kl_tensor(c), _klen(c)
    keep = _keep(c)
    o_ref, lse_ref, mag = _ref_forward(q, k, v, slopes, klc, keep, c.p)
    # ---- forward
    qkvb = Buf(rows, W + (0 if c.layout == "a" else 8), dt)
    _put(qkvb, 0, q.reshape(rows, H * 64))
    _put(qkvb, H * 64, k.reshape(rows, 64))
    _put(qkvb, H * 64 + 64, v.reshape(rows, 64))
    ob = _out_buf("d" if c.layout == "de" else "a", rows, H, dt)
    lseb = Buf(1, B * H * N, torch.float32)
    _call_train_fwd(c, qkvb, slopes, kl, ob, lseb)
    o_first, lse_first = ob.snapshot(), lseb.snapshot()
    o_got = ob.mat[:, :H * 64].reshape(B, N, H, 64)
    lse_got = lseb.mat.view(B, H, N)
    o_scale = o_ref.abs().max().item()
    err_o = _err(o_got, o_ref)
    _record(c.entry, "o", err_o / o_scale)
    tol_o = (5e-6 * _scale(mag) if f32 else 1e-2) * o_scale        # test_gpu_train.py: 5e-6 (fp32), 1e-2 (bf16 vs fp32)
    assert err_o <= tol_o, f"o: max |diff| {err_o:.3e} (tol {tol_o:.3e}, |m| {mag:.1f})"
    # lse: fp32 statistics in both pairs (row max + log of an fp32 sum): 1e-5 of the scale, as test_gpu_train.py's bf16-vs-fp32
    lse_scale = max(1.0, lse_ref.abs().max().item())
    err_l = _err(lse_got, lse_ref)
    _record(c.entry, "lse", err_l / lse_scale)
    assert err_l <= 1e-5 * lse_scale, f"lse: max |diff| {err_l:.3e} (scale {lse_scale:.3e})"
    ob.assert_outside_untouched(H * 64, "o")
    lseb.assert_outside_untouched(B * H * N, "lse")
    _call_train_fwd(c, qkvb, slopes, kl, ob, lseb)
    assert torch.equal(ob.snapshot(), o_first) and torch.equal(lseb.snapshot(), lse_first), "forward not reproducible"
    # ---- backward, on the o the forward returned
    g = torch.Generator(device=DEV).manual_seed(N * 131 + H)
    d_o = torch.randn((B, N, H, 64), generator=g, device=DEV).to(dt).double()
    if not c.dopad:       # training zeroes dO on padded query rows (the caller's row mask)
        d_o = d_o * (torch.arange(N, device=DEV)[None, :] < klc[:, None])[..., None, None]
    o_in = o_got.double()
    dq_ref, dk_ref, dv_ref, dls_ref = _ref_backward(q, k, v, slopes, klc, keep, c.p, o_in, d_o)
    ldo = H * 64 + (8 if c.layout == "de" else 0)
    oinb, dob = Buf(rows, ldo, dt), Buf(rows, ldo, dt)
    _put(oinb, 0, o_in.reshape(rows, H * 64))
    _put(dob, 0, d_o.reshape(rows, H * 64))
    dqb = Buf(rows, qkvb.ld, dt, 4 if c.layout == "de" else 0)
    dlsb = Buf(1, H, torch.float32)
    ws = torch.full((_ws_floats(c),), float("nan"), device=DEV)
    _call_train_bwd(c, qkvb, oinb, dob, slopes, kl, lseb, dqb, dlsb, ws)
    dq_first, dls_first = dqb.snapshot(), dlsb.snapshot()
    got = dqb.mat[:, :W]
    # fp32: test_gpu_train.py's bounds, 2e-5 (3e-5 with dropout) of the scale, 5e-5 (1e-4) for d log-slope.
    # bf16: 1e-2 / 2e-2 - the bounds the pair had against fp32, now against float64 (bf16 P, dS and outputs: 2^-9 each).
    # dQ, dK and dV are measured against the scale of the whole dqkv (as the fp32 dropout test does): dQ and dK can vanish in
    # float64 (one attended key: dS = P (dP - delta) = 0) while the kernels' dP - delta leaves fp32 / bf16 rounding.
    gscale = max(dq_ref.abs().max().item(), dk_ref.abs().max().item(), dv_ref.abs().max().item())
    base, base_s = (2e-5, 5e-5) if c.p == 0 else (3e-5, 1e-4)
    if not f32:
        base, base_s = 1e-2, 2e-2
    fac = _scale(mag) if f32 else 1.0
    for what, gv, rv in (("dQ", got[:, :H * 64].reshape(B, N, H, 64), dq_ref), ("dK", got[:, H * 64:H * 64 + 64], dk_ref.reshape(rows, 64)),
                         ("dV", got[:, H * 64 + 64:W], dv_ref.reshape(rows, 64)), ("dlogslope", dlsb.mat[0], dls_ref)):
        sc = max(rv.abs().max().item(), 1e-30) if what == "dlogslope" else gscale
        e = _err(gv, rv)
        _record(c.entry, what, e / sc)
        tol = (base_s if what == "dlogslope" else base) * fac
        assert e <= tol * sc, f"{what}: max |diff| {e:.3e} vs scale {sc:.3e} (tol {tol:g} relative, |m| {mag:.1f})"
    dqb.assert_outside_untouched(W, "dqkv")
    dlsb.assert_outside_untouched(H, "dlogslopes")
    ws.fill_(float("nan"))
    _call_train_bwd(c, qkvb, oinb, dob, slopes, kl, lseb, dqb, dlsb, ws)
    assert torch.equal(dqb.snapshot(), dq_first) and torch.equal(dlsb.snapshot(), dls_first), "backward not reproducible"


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_attention_matrix(c):
    if c.entry.startswith("train"):
        _run_training(c)
    else:
        _run_inference(c)


def test_matrix_reaches_every_branch_and_axis_value():
    """Bookkeeping of the matrix above: every dispatch branch and every listed axis value is reached per entry."""
    def have(entry, pred):
        return any(c.entry == entry and pred(c) for c in CASES)
    for e, hs in (("f32", range(1, 9)), ("bf16", range(1, 9)), ("split", range(1, 9)), ("train_f32", range(1, 9)),
                  ("train_bf16", range(1, 7))):
        for h in hs:
            assert have(e, lambda c: c.H == h), (e, h)
        for n in NS:
            assert have(e, lambda c: c.N == n), (e, n)
        for pat in PATTERNS:
            assert have(e, lambda c: c.lens == _lens(pat, c.N, c.B)), (e, pat)
        for edge in (31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513):
            assert have(e, lambda c: c.lens is not None and edge in c.lens and edge < c.N), (e, edge)
        for fam in ("spike_more", "spike_less", "big_slope"):
            assert have(e, lambda c: c.family == fam), (e, fam)
        for lay in ("a", "b", "c", "d") if not e.startswith("train") else ("a", "b", "de"):
            assert have(e, lambda c: c.layout == lay), (e, lay)
        if e.startswith("train"):
            for p in (0.0, 0.1, 0.3):
                assert have(e, lambda c: c.p == p), (e, p)
            assert have(e, lambda c: c.dopad)
            assert have(e, lambda c: c.N > 512 and c.lens is not None and any(512 < x < c.N for x in c.lens))
    assert have("train_f32", lambda c: not c.lse_in) and have("train_f32", lambda c: c.lse_in)
    branches = {_branch("bf16", c.B, c.N, c.H, c.qpw) for c in CASES if c.entry == "bf16"}
    for mi in ("<1024,4>", "<768,4>", "<768,8>", "<768,16>"):
        assert any(mi in b for b in branches), mi
    for q in (1, 2, 3, 4, 8):
        assert have("bf16", lambda c: c.qpw == q)
    assert have("bf16", lambda c: c.qpw > 1 and ((c.N + 63) // 64) % c.qpw != 0 and c.N <= 512)
    assert have("bf16", lambda c: c.qpw > (c.N + 63) // 64 and c.N <= 512)
    assert have("bf16", lambda c: c.qpw > 1 and c.N > 512)
    assert have("bf16", lambda c: c.qpw == 0 and _bf16_plan(c.B, c.N, c.H, 0)[2] > 1)
    assert {_branch("split", 1, 1, h, 0) for h in range(1, 9)} == {"split-one", "split-4+1", "split-6+1", "split-6+2"}




# ------------------------------------------------------------------------------------------------------- refusals
def _refusal(fn, args, out: Buf, words):
    before = out.snapshot()
    rc = fn(*args)
    torch.cuda.synchronize()
    msg = runtime.lib().ispk_last_error_string()
    msg = msg.decode() if msg else ""
    assert rc != 0, "accepted"
    assert any(w in msg for w in words), msg
    assert torch.equal(out.snapshot(), before), "refused call wrote its output"


def _inf_args(entry, B, N, H, dt, ldq=None, ldo=None, qoff=0, big=False):
    W = H * 64 + 128
    ldq = W if ldq is None else ldq
    inp = Buf(max(B * N, 1) if not big else 2, ldq, dt)
    inp.mat.zero_()
    out = Buf(max(B * N, 1) if not big else 2, H * 64 if ldo is None else ldo, dt)
    sl = torch.ones(max(H, 1), device=DEV)
    es = inp.back.element_size()
    L = runtime.lib()
    base = (inp.ptr() + qoff * es, ldq, inp.ptr(H * 64), inp.ptr(H * 64 + 64), ldq, sl.data_ptr(),
            None, out.ptr(), out.ld, B, N, H)
    fn = {"f32": L.ispk_alibi_mqa_attn_f32, "bf16": L.ispk_alibi_mqa_attn_bf16, "split": L.ispk_alibi_mqa_attn_split_f16}[entry]
    if entry == "split":
        base = base[:9] + (0,) + base[9:]
    return fn, base + (runtime._stream(),), out, (inp, sl)   # (inputs kept alive by the caller)


@pytest.mark.parametrize("entry", ["f32", "bf16", "split"])
def test_inference_entries_refuse_bad_arguments(entry):
    dt = torch.bfloat16 if entry == "bf16" else torch.float32
    H = 6
    W = H * 64 + 128
    bad_ld = W + (4 if entry == "bf16" else 2)
    for kw, words in ((dict(H=9), ("H=9",)), (dict(ldq=bad_ld), ("multiple",)), (dict(ldo=H * 64 + 2), ("multiple",)),
                      (dict(qoff=4 if entry == "bf16" else 1), ("aligned",)), (dict(B=65536, big=True), ("65535",))):
        a = dict(B=2, N=40, H=H)
        a.update(kw)
        fn, args, out, _inputs = _inf_args(entry, a["B"], a["N"], a["H"], dt, a.get("ldq"), a.get("ldo"), a.get("qoff", 0),
                                        a.get("big", False))
        _refusal(fn, args, out, words)


@pytest.mark.parametrize("entry", ["train_f32", "train_bf16"])
def test_training_entries_refuse_bad_arguments(entry):
    f32 = entry == "train_f32"
    dt = torch.float32 if f32 else torch.bfloat16
    L, st = runtime.lib(), runtime._stream()
    fwd = L.ispk_alibi_mqa_attn_train_f32 if f32 else L.ispk_alibi_mqa_attn_train_bf16
    B, N, H = 2, 40, 4
    W = H * 64 + 128
    qkv = Buf(B * N, W + 8, dt)
    qkv.mat.zero_()
    sl = torch.ones(8, device=DEV)
    h_bad = 9 if f32 else 7
    for over, words in ((dict(H=h_bad), (f"H={h_bad}",)), (dict(ld_qkv=W + (2 if f32 else 4)), ("bad shape", "ld_qkv")),
                        (dict(ld_o=H * 64 + 2), ("bad shape", "ld_o")), (dict(qoff=4 if not f32 else 1), ("aligned",)),
                        (dict(B=65536), ("bad shape",)), (dict(p=1.0), ("dropout_p",))):
        a = dict(B=B, H=H, ld_qkv=qkv.ld, ld_o=H * 64, qoff=0, p=0.1)
        a.update(over)
        o = Buf(B * N, max(a["ld_o"], 8 * 64), dt)
        lse = Buf(1, B * 8 * N, torch.float32)
        _refusal(fwd, (qkv.ptr(a["qoff"]), a["ld_qkv"], sl.data_ptr(), None, o.ptr(), a["ld_o"], lse.ptr(), a["B"], N, a["H"],
                       a["p"], 1, st), o, words)
    # backward: the same, plus a workspace one float short
    o_in, d_o = Buf(B * N, H * 64, dt), Buf(B * N, H * 64, dt)
    o_in.mat.zero_()
    d_o.mat.zero_()
    lse = Buf(1, B * H * N, torch.float32)
    lse.mat.zero_()
    need = (2 * B * H * N + H * B * ((N + 31) // 32)) if f32 else (B * H * N + 2 * H * B * ((N + 63) // 64))
    ws = torch.zeros(need + 1, device=DEV)
    dls = Buf(1, 8, torch.float32)

    def bwd(B_, H_, ld_qkv, ld_o, qoff, p, wsf, dq):
        if f32:
            return L.ispk_alibi_mqa_attn_bwd_f32(qkv.ptr(qoff), ld_qkv, o_in.ptr(), d_o.ptr(), ld_o, sl.data_ptr(), None, dq.ptr(),
                                                 dls.ptr(), ws.data_ptr(), wsf, B_, N, H_, lse.ptr(), p, 1, st)
        return L.ispk_alibi_mqa_attn_bwd_bf16(qkv.ptr(qoff), ld_qkv, o_in.ptr(), d_o.ptr(), ld_o, sl.data_ptr(), None, lse.ptr(),
                                              dq.ptr(), dls.ptr(), ws.data_ptr(), wsf, B_, N, H_, p, 1, st)
    for over, words in ((dict(H_=h_bad), (f"H={h_bad}",)), (dict(ld_qkv=W + (2 if f32 else 4)), ("bad shape", "ld_qkv")),
                        (dict(ld_o=H * 64 + (2 if f32 else 4)), ("bad shape", "ld_o")),
                        (dict(qoff=4 if not f32 else 1), ("aligned",)), (dict(wsf=need - 1), ("workspace",)),
                        (dict(B_=65536), ("bad shape",)), (dict(p=1.0), ("dropout_p",))):
        a = dict(B_=B, H_=H, ld_qkv=qkv.ld, ld_o=H * 64, qoff=0, p=0.1, wsf=need)
        a.update(over)
        dq = Buf(B * N, qkv.ld, dt)
        _refusal(bwd, tuple(a[k] for k in ("B_", "H_", "ld_qkv", "ld_o", "qoff", "p", "wsf")) + (dq,), dq, words)


# ------------------------------------------------------------------------------------------------------- empty batches
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_wrappers_return_empty_results_for_an_empty_batch(dt):
    """torch gives an empty tensor a NULL data_ptr() and the C entries check pointers first: the wrappers must not call them."""
    H, N = 4, 50
    qkv = torch.zeros((0, N, H * 64 + 128), dtype=dt, device=DEV)
    sl = torch.ones(H, device=DEV)
    kl = torch.zeros((0,), dtype=torch.int64, device=DEV)
    for key_len in (None, kl):
        o = runtime.alibi_mqa_attention(qkv, H, sl, key_len)
        assert o.shape == (0, N, H * 64) and o.dtype == dt
        if dt == torch.bfloat16:
            assert runtime.alibi_mqa_attention(qkv, H, sl, key_len, q_tiles=2).shape == (0, N, H * 64)
        else:
            assert runtime.alibi_mqa_attention_split(qkv, H, sl, key_len).shape == (2, 0, N, H * 64)
            assert runtime.alibi_mqa_attention_split(qkv, H, sl, key_len, out_split=False).shape == (0, N, H * 64)
        o, lse = runtime.alibi_mqa_attention_train(qkv, H, sl, key_len, 0.1, 3)
        assert o.shape == (0, N, H * 64) and lse.shape == (0, H, N)
        for lse_in in ((lse,) if dt == torch.bfloat16 else (None, lse)):
            dqkv, dls = runtime.alibi_mqa_attention_bwd(qkv, o, o, H, sl, key_len, lse=lse_in, dropout_p=0.1, seed=3)
            assert dqkv.shape == qkv.shape and dqkv.dtype == dt
            assert dls.shape == (H,) and torch.equal(dls, torch.zeros_like(dls))
