"""CPU: `plan.short_block_ok`, the predicate `Attention.forward` consults before it launches the attention block as one kernel
(ispk_attn_block_short_bf16), over dtype, positions, dims, `defer_out`, tape, residual and the row threshold - and that
`Attention` carries the switch, default on."""
import itertools

import torch

from isp_tts_amd.modules.transformer import plan
from isp_tts_amd.modules.transformer.attention import Attention

OK = dict(cdt=torch.bfloat16, tape=False, residual=True, defer_out=False, n=100, heads=6, dim=384, out_dim=384, rows=6400)


def test_the_benchmark_shapes_qualify():
    assert plan.short_block_ok(**OK)
    assert plan.short_block_ok(**dict(OK, heads=4, dim=256, out_dim=256))


def test_each_condition_alone_turns_it_off():
    for change in (dict(cdt=torch.float32), dict(cdt=torch.float16), dict(tape=True), dict(residual=False), dict(defer_out=True),
                   dict(n=129), dict(n=0), dict(heads=5), dict(heads=8, dim=512, out_dim=512), dict(heads=2, dim=128, out_dim=128),
                   dict(dim=256, out_dim=256), dict(out_dim=256), dict(rows=plan.SHORT_BLOCK_MIN_ROWS[384] - 1)):
        assert not plan.short_block_ok(**dict(OK, **change)), change


def test_positions_and_rows_at_the_thresholds():
    assert plan.SHORT_BLOCK_MAX_N == 128
    for n in (1, 32, 33, 64, 65, 127, 128):
        assert plan.short_block_ok(**dict(OK, n=n))
    for dim, heads in ((384, 6), (256, 4)):
        lo = plan.SHORT_BLOCK_MIN_ROWS[dim]
        assert lo >= 1
        assert plan.short_block_ok(**dict(OK, heads=heads, dim=dim, out_dim=dim, rows=lo))
        assert not plan.short_block_ok(**dict(OK, heads=heads, dim=dim, out_dim=dim, rows=lo - 1))


def test_the_predicate_is_a_conjunction():
    """Any combination of failing conditions fails; only all-good passes."""
    bad = [dict(cdt=torch.float32), dict(tape=True), dict(defer_out=True), dict(n=200)]
    for k in range(1, len(bad) + 1):
        for combo in itertools.combinations(bad, k):
            kw = dict(OK)
            for c in combo:
                kw.update(c)
            assert not plan.short_block_ok(**kw)


def test_attention_carries_the_switch_and_the_tape_test():
    att = Attention(dim=384, heads=6, one_kv_head=True, alibi_pos_bias=True)
    assert att.short_block is True
    assert not att._no_tape()                      # trainable parameters, gradients enabled: the training forward's tape
    with torch.no_grad():
        assert att._no_tape()
    assert att.requires_grad_(False)._no_tape()
