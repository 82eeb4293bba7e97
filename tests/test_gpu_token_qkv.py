"""GPU: the text encoder's first attention_norm + q/kv projection as a per-token table (`AcousticModel.token_qkv_table`):
`ispk_embed_tokens_qkv` against `embed_tokens` and LayerNorm + GEMM over the gathered rows.  The model with the switch off / on
and the table's staleness check: tests/test_gpu_model_handoffs.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from isp_tts_amd import runtime, synth  # noqa: E402

DEV = "cuda"


def _bf(t):
    return t.to(torch.bfloat16)


def test_embed_tokens_qkv_against_the_launches_it_replaces():
    """B = 2, L = 9, ids 0, 148, -1 and 149 among them (outside [0, vocab): row 0): emb and mask equal `embed_tokens`' bit for bit;
    q/kv rows against LayerNorm (bf16 out) + GEMM over the gathered rows and against float64, at the bounds the project holds its
    other q/kv epilogue to (tests/test_gpu_kernels.py: max <= 2^-5 and rms <= 2e-3 vs the launches, max <= 0.08 vs float64)."""
    V, D, N = 149, 384, 512
    table = synth._normal("t/tq/table", (V, D), 1.5, 0.4)
    g, b = synth._normal("t/tq/g", (D,), 0.1, 1.0), synth._normal("t/tq/b", (D,), 0.1)
    wq = _bf(synth._normal("t/tq/wq", (N, D), D ** -0.5))
    text = torch.tensor([[0, 148, -1, 149, 5, 77, 148, 1, 0], [3, 3, 120, 0, 0, 0, 0, 0, 0]], dtype=torch.int64)
    text_len = torch.tensor([9, 3])
    d = lambda t: t.to(DEV)  # noqa: E731
    qkv_table = runtime.gemm(runtime.layernorm(d(table), d(g), d(b), eps=1e-5, out_dtype=torch.bfloat16), d(wq))
    assert qkv_table.shape == (V, N) and qkv_table.dtype == torch.bfloat16
    emb0, mask0 = runtime.embed_tokens(d(text), d(table), d(text_len))
    emb, mask, qkv = runtime.embed_tokens_qkv(d(text), d(table), qkv_table, d(text_len))
    emb2, mask2, qkv2 = runtime.embed_tokens_qkv(d(text), d(table), qkv_table, d(text_len))
    assert torch.equal(emb, emb0) and torch.equal(mask, mask0)
    assert torch.equal(emb, emb2) and torch.equal(mask, mask2) and torch.equal(qkv, qkv2)
    assert qkv.shape == (2, 9, N) and qkv.dtype == torch.bfloat16
    ids = torch.where((text < 0) | (text >= V), torch.zeros_like(text), text)
    assert torch.equal(emb.cpu(), table[ids])
    two = runtime.gemm(runtime.layernorm(emb0, d(g), d(b), eps=1e-5, out_dtype=torch.bfloat16), d(wq)).cpu().float()
    e2 = (qkv.cpu().float() - two).abs()
    x64 = table[ids].double()
    hn = (x64 - x64.mean(-1, keepdim=True)) / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + 1e-5) * g.double() + b.double()
    e64 = (qkv.cpu().double() - hn @ wq.double().t()).abs()
    print(f"token q/kv: vs LayerNorm + GEMM max {e2.max().item():.3e} rms {e2.pow(2).mean().sqrt().item():.3e}; "
          f"vs float64 max {e64.max().item():.3e}")
    assert e2.max().item() <= 2 ** -5 and e2.pow(2).mean().sqrt().item() <= 2e-3 and e64.max().item() <= 0.08
    # no mask wanted, no lengths (batch-1 infer)
    emb3, none, qkv3 = runtime.embed_tokens_qkv(d(text), d(table), qkv_table, None, want_mask=False)
    assert none is None and torch.equal(emb3, emb) and torch.equal(qkv3, qkv)
