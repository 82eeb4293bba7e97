"""GPU: `Attention.short_block` in the stacks that take it on the bf16 no-tape forward - a text-encoder stack (depth 2, dim 384, 6
heads) and an adaptive dim-256 stack (4 heads: the flow predictor's kind of layer) at B = 2 x N = 100.  Switch on against off: the
stack's output and every layer's q/kv intermediates are torch.equal, the launches are the one kernel instead of the three; at
N = 129, on the fp32 path and below `plan.SHORT_BLOCK_MIN_ROWS` the switch changes nothing.  (200 rows are below the dim-256
threshold, which is a speed choice: the equality tests move it to 1 to reach the kernel.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from isp_tts_amd import runtime, synth  # noqa: E402
from isp_tts_amd.config import AcousticDims  # noqa: E402
from isp_tts_amd.modules.transformer import plan  # noqa: E402
from isp_tts_amd.modules.transformer.transformer import Transformer  # noqa: E402

DEV = "cuda"
BLOCK = {384: "attn_block_short_kernel<6>", 256: "attn_block_short_kernel<4>"}


def _stack(kind):
    cfg = AcousticDims().model_config()
    torch.manual_seed(11)
    if kind == "encoder":
        tr = Transformer.init(dict(cfg["encoder"], depth=2), emb_dim=384)
    else:
        tr = Transformer.init(dict(cfg["temporal_adaptor"]["predictor"]["transformer"], depth=1), emb_dim=256, adaptive_norm=True,
                              condition_dim=32)
    with torch.no_grad():      # (learned slopes and norm parameters away from their initial values)
        for name, p in tr.named_parameters():
            if p.dim() == 1:
                p.add_(synth._normal(f"t/abm/{kind}/{name}", tuple(p.shape), 0.1))
    return tr.eval().to(DEV).requires_grad_(False).set_compute_dtype(torch.bfloat16)


def _run(tr, x, mask, cond, on):
    for layer in tr.layers:
        layer.attention.short_block = on
    tr(x, mask=mask, adaptive_condition=cond)      # (stages the weight images: their one-time launches are not counted)
    prof = runtime.LaunchProfiler()
    runtime.set_profiler(prof)
    try:
        out = tr(x, mask=mask, adaptive_condition=cond, return_intermediates=True)
        torch.cuda.synchronize()
    finally:
        runtime.set_profiler(None)
        for layer in tr.layers:
            layer.attention.short_block = True
    return out, [r[0] for r in prof.records]


def _inputs(kind, N):
    dim = 384 if kind == "encoder" else 256
    x = synth._normal(f"t/abm/x/{kind}/{N}", (2, N, dim)).to(DEV)
    lens = torch.tensor([N, N // 2 + 3], device=DEV)
    mask = torch.arange(N, device=DEV)[None, :] < lens[:, None]
    cond = synth._normal(f"t/abm/c/{kind}", (2, 1, 32)).to(DEV) if kind == "adaptive" else None
    return x * mask[..., None], mask, cond


def _same(a, b):
    assert torch.equal(a.out, b.out)
    assert len(a.intermediates) == len(b.intermediates) > 0
    for ia, ib in zip(a.intermediates, b.intermediates):
        for name in ("queries", "keys", "values"):
            assert torch.equal(getattr(ia.attention, name), getattr(ib.attention, name)), name


@pytest.mark.parametrize("kind", ("encoder", "adaptive"))
def test_stack_with_the_switch_on_equals_off(kind, monkeypatch):
    monkeypatch.setitem(plan.SHORT_BLOCK_MIN_ROWS, 256, 1)
    tr = _stack(kind)
    x, mask, cond = _inputs(kind, 100)
    on, l_on = _run(tr, x, mask, cond, True)
    off, l_off = _run(tr, x, mask, cond, False)
    depth, label = len(tr.layers), BLOCK[tr.dim]
    assert l_on.count(label) == depth and label not in l_off
    assert sum(l.startswith("attn_bf16_kernel") for l in l_off) == depth and not any(l.startswith("attn_bf16_kernel") for l in l_on)
    # per layer: q/kv GEMM + attention + to_out GEMM -> one launch (a layer whose q/kv rows were handed to it had no q/kv GEMM)
    assert len(l_off) - len(l_on) == 2 * depth
    assert torch.isfinite(on.out).all()
    _same(on, off)


@pytest.mark.parametrize("kind", ("encoder", "adaptive"))
def test_longer_sequences_and_fp32_take_the_three_launches(kind, monkeypatch):
    monkeypatch.setitem(plan.SHORT_BLOCK_MIN_ROWS, 256, 1)
    tr = _stack(kind)
    x, mask, cond = _inputs(kind, 129)
    on, l_on = _run(tr, x, mask, cond, True)
    off, l_off = _run(tr, x, mask, cond, False)
    assert l_on == l_off and not any(l.startswith("attn_block_short") for l in l_on)
    assert sum(l.startswith("attn_bf16_kernel") for l in l_on) == len(tr.layers)
    _same(on, off)
    tr.set_compute_dtype(torch.float32)
    x, mask, cond = _inputs(kind, 100)
    _, l32 = _run(tr, x, mask, cond, True)
    assert not any(l.startswith("attn_block_short") for l in l32)


def test_rows_below_the_threshold_take_the_three_launches():
    """200 rows at dim 256: below `SHORT_BLOCK_MIN_ROWS[256]`, the switch on launches what off launches."""
    assert plan.SHORT_BLOCK_MIN_ROWS[256] > 200
    tr = _stack("adaptive")
    x, mask, cond = _inputs("adaptive", 100)
    on, l_on = _run(tr, x, mask, cond, True)
    off, l_off = _run(tr, x, mask, cond, False)
    assert l_on == l_off and not any(l.startswith("attn_block_short") for l in l_on)
    _same(on, off)
