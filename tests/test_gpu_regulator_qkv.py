"""GPU: `ispk_length_regulate_qkv_bf16` - the bf16 path's length regulator with the consuming layer's attention_norm + q/kv
projection as its epilogue - against the unfused entry point (bit for bit on what both write), `gemm_lnin` on its rows and float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from isp_tts_amd import runtime, synth  # noqa: E402

DEV = "cuda"
B, L, M, D, N = 3, 37, 150, 384, 512        # L: not a multiple of the 16-token chunk; M: a partial last frame tile
TEXT_LEN, MEL_LEN = (37, 20, 1), (150, 64, 9)


def _case(B, L, M, text_len, mel_len):
    x = synth._normal(f"t/lrq/x{B}", (B, L, D), 1.5, 0.4)
    g, b = synth._normal("t/lrq/g", (D,), 0.1, 1.0), synth._normal("t/lrq/b", (D,), 0.1)
    wq = synth._normal("t/lrq/wq", (N, D), D ** -0.5).to(torch.bfloat16)
    text_len, mel_len = torch.tensor(text_len), torch.tensor(mel_len)
    tm = torch.arange(L)[None] < text_len[:, None]
    mm = torch.arange(M)[None] < mel_len[:, None]
    logits = synth._normal(f"t/lrq/a{B}", (B, M, L), 3.0).masked_fill(~tm[:, None], float("-inf"))
    attn = torch.softmax(logits, dim=-1) * mm[..., None]            # the aligner's attn_soft: rows past mel_len are zero
    dur = torch.from_numpy(synth._rng(f"t/lrq/d{B}").random((B, L)).astype("float32")) + 0.05
    dur = dur * tm
    dur = dur * ((mel_len.float() - 0.25) / dur.sum(1))[:, None]      # fractional durations: floor(sum + 0.5) = mel_len
    return {k: v.to(DEV) for k, v in dict(x=x, g=g, b=b, wq=wq, text_len=text_len, mel_len=mel_len, attn=attn, dur=dur).items()}


@pytest.fixture(scope="module")
def case():
    return _case(B, L, M, TEXT_LEN, MEL_LEN)


def _check(c, source, B, M, mel_len):
    """From `attn_soft` or from the soft path generated in the kernel; twice.  out, dec_len and dec_mask equal the unfused entry point's bit for bit, q/kv is the same on both runs; q/kv
    against `gemm_lnin(out, None, ...)` - the launch it replaces - and float64 at the bounds of the feed-forward kernel's q/kv
    epilogue (tests/test_gpu_kernels.py): max <= 2^-5, rms <= 2e-3; max <= 0.08 vs float64.  Every row, those past dec_len too."""
    wqc = runtime.chunk_k16(c["wq"])
    if source == "attn_soft":
        args = (c["x"], c["mel_len"].view(-1, 1), c["attn"], M)
        kw = dict(max_len=M, split_bf16=True)
    else:
        args = (c["x"], c["dur"], None, M)
        kw = dict(max_len=M, enc_len=c["text_len"], split_bf16=True)
    out0, len0, mask0 = runtime.length_regulate(*args, **kw)
    out, dec_len, mask, qkv = runtime.length_regulate(*args, next_qkv=(c["g"], c["b"], 1e-5, wqc), **kw)
    out2, dec_len2, mask2, qkv2 = runtime.length_regulate(*args, next_qkv=(c["g"], c["b"], 1e-5, wqc), **kw)
    assert torch.equal(out, out0) and torch.equal(dec_len, len0) and torch.equal(mask, mask0)
    assert torch.equal(out2, out0) and torch.equal(dec_len2, len0) and torch.equal(mask2, mask0) and torch.equal(qkv, qkv2)
    assert dec_len.tolist() == list(mel_len)
    assert qkv.dtype == torch.bfloat16 and qkv.shape == (B, M, N)
    two = runtime.gemm_lnin(out0, None, c["g"], c["b"], c["wq"]).cpu().float()
    eq = (qkv.cpu().float() - two).abs()
    o64 = out0.cpu().double()
    hn = (o64 - o64.mean(-1, keepdim=True)) / torch.sqrt(o64.var(-1, unbiased=False, keepdim=True) + 1e-5) * c["g"].cpu().double() \
        + c["b"].cpu().double()
    e64 = (qkv.cpu().double() - hn @ c["wq"].cpu().double().t()).abs()
    print(f"regulator q/kv ({source}): vs gemm_lnin max {eq.max().item():.3e} rms {eq.pow(2).mean().sqrt().item():.3e}; "
          f"vs float64 max {e64.max().item():.3e}")
    assert eq.max().item() <= 2 ** -5 and eq.pow(2).mean().sqrt().item() <= 2e-3 and e64.max().item() <= 0.08


@pytest.mark.parametrize("source", ["attn_soft", "soft_path"])
def test_regulator_with_the_qkv_epilogue(case, source):
    """B = 3, L = 37, M = 150, text_len (37, 20, 1), mel_len (150, 64, 9), from `attn_soft` and from the soft path generated in
    the kernel; twice (`_check`)."""
    _check(case, source, B, M, MEL_LEN)


@pytest.mark.parametrize("source", ["attn_soft", "soft_path"])
def test_regulator_with_the_qkv_epilogue_across_a_full_run_of_utterances(source):
    """B = 9, L = 5, M = 70 (two frame tiles): the first eight utterances' tiles take the one-XCD-per-utterance block mapping, the
    ninth (a ragged last run) the plain one - no result depends on it."""
    lens_t, lens_m = (5, 4, 3, 2, 1, 5, 5, 1, 3), (70, 64, 65, 1, 9, 33, 70, 2, 66)
    _check(_case(9, 5, 70, lens_t, lens_m), source, 9, 70, lens_m)
