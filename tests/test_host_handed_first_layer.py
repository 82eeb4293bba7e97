"""CPU: a stack whose caller hands layer 0 its q/kv rows (`Transformer.forward(handed=Handed(Hand.QKV, rows))`: the text encoder
behind the token q/kv table) plans that layer like any layer behind a producing one - and nothing else about the layer moves."""
import torch

from isp_tts_amd.modules.transformer.plan import Form, Hand, Next, Plan, Qkv, select_plan

FACTS = dict(cdt=torch.bfloat16, dim=384, heads=6, out_dim=384, inner=1536, plain_norms=True, bias1=False, bias2=False, gelu=True,
             dropout=False, consumer=Next.LAYER, next_heads=6, next_dim=384)


def test_first_layer_takes_handed_qkv_rows_and_keeps_the_rest_of_its_plan():
    # the pinned plans of layer 0 (tests/test_host_logic.py: 6,400 rows = the text encoder, 32,768 = the decoder)
    pinned = {6400: Plan(Qkv.NORM_GEMM, False, Form.SPLIT, 4, Hand.ROWS, torch.bfloat16),
              32768: Plan(Qkv.LNIN_SELF, True, Form.ATTN_OUT_FFN_QKV, 0, Hand.QKV)}
    for rows, plan in pinned.items():
        assert select_plan(rows=rows, **FACTS) == plan
        handed = select_plan(rows=rows, prev=Hand.QKV, **FACTS)
        assert handed.qkv is Qkv.HANDED_QKV
        assert handed[1:] == plan[1:]
