"""GPU: the hand-offs between the stacks on the bf16 no-tape forward - the token q/kv table (`AcousticModel.token_qkv_table`) and the
length regulator's q/kv epilogue (`LengthRegulator.hand_qkv`) - each switch off / on in the model (B = 2, L = 12, M = 40), the
table's staleness check, and one graphed forward with both on."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from isp_tts_amd import runtime, staging, synth  # noqa: E402

DEV = "cuda"
BF16_MEL_TOL = 6e-2      # tests/test_gpu_model.py: the bf16 path against the fp32 path

# switch -> (owner of the attribute, launches with it off, launches with it on)
SWITCHES = {
    "token_qkv_table": (lambda m: m, ["embed_tokens_kernel"], ["embed_tokens_qkv_kernel"]),
    "hand_qkv": (lambda m: m.temporal_adaptor.length_regulator, ["length_regulate_kernel<bf16x3>"], ["length_regulate_qkv_kernel"]),
}
REMOVED = {"token_qkv_table": 2, "hand_qkv": 2}     # launches a step loses with the switch on


def _inputs():
    inp = synth.make_inputs(2, 12, 40, seed=7)
    text_len, mel_len = torch.tensor([12, 7]), torch.tensor([40, 29])
    tm = torch.arange(12)[None] < text_len[:, None]
    mm = torch.arange(40)[None] < mel_len[:, None]
    return {k: v.to(DEV) for k, v in dict(
        text=inp["text"] * tm, text_len=text_len, mel=inp["mel"] * mm[:, None], mel_len=mel_len, pitch=inp["pitch"] * mm,
        energy=inp["energy"] * mm, flow_noise=inp["flow_x0"], flow_time=inp["flow_t"]).items()}


def _labels(model, inp):
    prof = runtime.LaunchProfiler()
    runtime.set_profiler(prof)
    try:
        model(**inp)
        torch.cuda.synchronize()
    finally:
        runtime.set_profiler(None)
    return [r[0] for r in prof.records]


@pytest.fixture(scope="module")
def fp32_mel(gpu_model):
    return gpu_model(**_inputs()).mel.clone()


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_model_with_each_switch_off_and_on(gpu_model, fp32_mel, switch):
    """With the switch off the launches are the separate ones, with it on they are gone; the hard alignment, the durations, the
    decoder lengths and the masks are equal, mel stays within the bf16 path's bound of the fp32 path's (and of the other
    setting's); the fp32 and split-fp16 paths never take the new kernels."""
    inp = _inputs()
    owner_of, off_labels, on_labels = SWITCHES[switch]
    owner = owner_of(gpu_model)
    assert getattr(owner, switch) is True
    new = [l for _, _, on in SWITCHES.values() for l in on]
    try:
        for dtype in (torch.float32, torch.float16):
            gpu_model.set_compute_dtype(dtype)
            assert not set(_labels(gpu_model, inp)) & set(new)
        gpu_model.set_compute_dtype(torch.bfloat16)
        setattr(owner, switch, False)
        off = gpu_model(**inp)
        l_off = _labels(gpu_model, inp)
        setattr(owner, switch, True)
        on = gpu_model(**inp)
        l_on = _labels(gpu_model, inp)
        assert all(l in l_off for l in off_labels) and not any(l in l_off for l in on_labels)
        assert all(l in l_on for l in on_labels) and not any(l in l_on for l in off_labels)
        assert len(l_on) == len(l_off) - REMOVED[switch]
        assert torch.equal(on.aligner_output.attn_hard, off.aligner_output.attn_hard)
        assert torch.equal(on.aligner_output.attn_hard_duration, off.aligner_output.attn_hard_duration)
        assert torch.equal(on.adaptor_output.dec_lengths, off.adaptor_output.dec_lengths)
        assert torch.equal(on.adaptor_output.dec_mask, off.adaptor_output.dec_mask)
        e_on, e_off = (on.mel - fp32_mel).abs().max().item(), (off.mel - fp32_mel).abs().max().item()
        e = (on.mel - off.mel).abs().max().item()
        print(f"{switch}: mel on vs fp32 {e_on:.3e}, off vs fp32 {e_off:.3e}, on vs off {e:.3e}")
        assert e_on < BF16_MEL_TOL and e_off < BF16_MEL_TOL and e < BF16_MEL_TOL
    finally:
        setattr(owner, switch, True)
        gpu_model.set_compute_dtype(torch.float32)


def test_graphed_forward_with_every_switch_on_and_the_table_rebuilt_after_a_weight_changes(gpu_model):
    """Both switches on: a graphed forward gives the eager one bit for bit.  A weight the token table is built from changes in
    place: the table is rebuilt at the next forward and the graph, which points at the old one, refuses to replay."""
    from isp_tts_amd.graph import GraphedForward
    inp = _inputs()
    try:
        gpu_model.set_compute_dtype(torch.bfloat16)
        on = gpu_model(**inp)
        labels = _labels(gpu_model, inp)
        assert all(l in labels for _, _, new in SWITCHES.values() for l in new)
        g = GraphedForward(gpu_model, inp["text"], inp["text_len"], inp["mel"], inp["mel_len"], inp["pitch"], inp["energy"],
                           inp["flow_noise"], inp["flow_time"])
        out = g.replay()
        assert torch.equal(out.mel, on.mel) and torch.equal(out.aligner_output.attn_hard, on.aligner_output.attn_hard)
        table = gpu_model._cache._slots["token_qkv"][1]
        before, n = table.clone(), staging.replacements()
        w = gpu_model.encoder.layers[0].attention_norm.weight
        saved = w.detach().clone()
        with torch.no_grad():
            w.mul_(1.25)
        changed = gpu_model(**inp)
        assert staging.replacements() > n and not torch.equal(gpu_model._cache._slots["token_qkv"][1], before)
        assert not torch.equal(changed.mel, on.mel)
        with pytest.raises(RuntimeError, match="rebuilt after this graph was captured"):
            g.replay()
        with torch.no_grad():
            w.copy_(saved)
        assert torch.equal(gpu_model(**inp).mel, on.mel)
        assert torch.equal(gpu_model._cache._slots["token_qkv"][1], before)
    finally:
        gpu_model.set_compute_dtype(torch.float32)
