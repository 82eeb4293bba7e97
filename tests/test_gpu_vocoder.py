"""GPU: the Vocos vocoder (isp_tts_amd.vocoder.Vocoder: csrc/vocoder.hip + the GEMM / LayerNorm entry points) against the
float64 module of tests/vocos_reference.py, run utterance by utterance, for the batch semantics (lengths, padding, NaN),
determinism, graph capture (alone and behind AcousticModel.infer), the absence of ATen compute, and the notebook's call.

Bounds, per utterance, over its samples m < 256 mel_len:
  fp32   max |audio - ref64| <= 1e-4 x max |ref64|
  bf16   max |audio - ref64| <= BF16_FACTOR x max |ref_bf16 - ref64|, ref_bf16 = the float64 module with every GEMM operand
         rounded to bf16 on the CPU (vocos_reference.forward_bf16_operands), the way tests/amp_bounds.py states its bounds
and exactly 0 at and past 256 mel_len."""
import math

import pytest
import torch

import vocos_reference as vr
from isp_tts_amd import graph, runtime, synth
from isp_tts_amd.vocoder import Vocoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_REL = 1e-4
BF16_FACTOR = 3.0

# name -> (dims, B, T, lengths or None, strided)
CASES = {
    "b1_t1": (1, 1, None, False), "b1_t2": (1, 2, None, False), "ragged": (3, 64, [1, 7, 64], False),
    "zero_len": (4, 17, [5, 0, 17, 9], False), "long": (2, 1723, [1723, 1500], False), "bench": (64, 512, None, False),
    "strided": (2, 40, [40, 31], True),
}
DIMS = ("official", "small")


def _mel(dims: str, case: str) -> tuple[torch.Tensor, torch.Tensor]:
    B, T, lens, strided = CASES[case]
    n_mels = synth.VOCODER_DIMS[dims][0]
    mel = synth.make_vocoder_mel(B, n_mels, T, seed=len(case))
    if strided:    # [B, C, T] view of [B, T, C] storage
        mel = mel.transpose(1, 2).contiguous().transpose(1, 2)
    ml = torch.tensor(lens if lens is not None else [T] * B, dtype=torch.int64)
    return mel, ml


@pytest.fixture(scope="module")
def models():
    out = {}
    for d in DIMS:
        sd = synth.make_vocoder_state_dict(synth.VOCODER_DIMS[d])
        out[d] = (sd, vr.build(sd), Vocoder.from_state_dict(sd).to(DEV).eval())
    return out


@pytest.fixture(scope="module")
def refs(models):
    """(dims, case) -> (ref64, ref_bf16): computed once, shared by the fp32 and bf16 tests."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cache = {}

    def get(d, case):
        if (d, case) not in cache:
            mel, ml = _mel(d, case)
            m = models[d][1]
            cache[(d, case)] = (vr.run_batch(m, mel, ml), vr.run_batch(m, mel, ml, vr.forward_bf16_operands))
        return cache[(d, case)]
    return get


def _run(voc: Vocoder, mel, ml, dtype=torch.float32, lengths=True):
    voc.set_compute_dtype(dtype)
    try:
        audio, alen = voc(mel.to(DEV), ml.to(DEV) if lengths else None)
        torch.cuda.synchronize()
    finally:
        voc.set_compute_dtype(torch.float32)
    return audio.cpu(), alen.cpu()


def _check_padding(audio, alen, ml):
    assert torch.equal(alen, ml * 256)
    for b in range(audio.shape[0]):
        assert (audio[b, int(alen[b]):] == 0).all(), f"utterance {b}: non-zero samples past audio_len"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dims", DIMS)
def test_fp32_against_float64(models, refs, dims, case):
    mel, ml = _mel(dims, case)
    ref64, _ = refs(dims, case)
    audio, alen = _run(models[dims][2], mel, ml, lengths=CASES[case][2] is not None)
    _check_padding(audio, alen, ml)
    worst = 0.0
    for b in range(mel.shape[0]):
        n = 256 * int(ml[b])
        if n == 0:
            continue
        peak = float(ref64[b, :n].abs().max())
        err = float((audio[b, :n].double() - ref64[b, :n]).abs().max())
        worst = max(worst, err / peak)
        assert err <= FP32_REL * peak, f"{dims}/{case} utterance {b}: max err {err:.3e} > 1e-4 x peak {peak:.3e}"
    print(f"{dims}/{case}: fp32 worst max|err| / peak = {worst:.2e}")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dims", DIMS)
def test_bf16_against_float64_with_bf16_operands(models, refs, dims, case):
    mel, ml = _mel(dims, case)
    ref64, ref_bf = refs(dims, case)
    audio, alen = _run(models[dims][2], mel, ml, torch.bfloat16, lengths=CASES[case][2] is not None)
    _check_padding(audio, alen, ml)
    worst = 0.0
    for b in range(mel.shape[0]):
        n = 256 * int(ml[b])
        if n == 0:
            continue
        rounding = float((ref_bf[b, :n] - ref64[b, :n]).abs().max())
        err = float((audio[b, :n].double() - ref64[b, :n]).abs().max())
        worst = max(worst, err / rounding)
        assert err <= BF16_FACTOR * rounding, f"{dims}/{case} utterance {b}: bf16 err {err:.3e} > {BF16_FACTOR} x {rounding:.3e}"
    print(f"{dims}/{case}: bf16 worst err / bf16-operand error = {worst:.2f}")


# ------------------------------------------------------------------------------------------------ the ISTFT head alone
def _head_rows(spec: torch.Tensor, ldh: int = 1032) -> torch.Tensor:
    """complex [513, T] -> fp32 rows [T, ldh]: log|X| in columns 0-512, angle X in 513-1025."""
    h = torch.zeros((spec.shape[1], ldh), dtype=torch.float32)
    h[:, :513] = spec.abs().log().T.float()
    h[:, 513:1026] = spec.angle().T.float()
    return h


def _head(h_rows: torch.Tensor, T: int, ml: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    B = ml.shape[0]
    tables = Vocoder(80, 64, 64, 1).tables().to(DEV)
    audio = torch.full((B, 256 * T + 100), 7.0, device=DEV)          # S > 256 T: the tail must be zeroed
    alen = torch.empty((B,), dtype=torch.int64, device=DEV)
    runtime.istft_head(h_rows.to(DEV), T, ml.to(DEV), tables, audio, alen)
    torch.cuda.synchronize()
    return audio.cpu(), alen.cpu()


def test_istft_head_analysis_synthesis():
    """Same-framed STFTs of clips with ragged lengths, fed as [log|X|, angle X], come back to 1e-5 of their peak."""
    T = 48
    lens = [48, 17, 1]
    window = torch.hann_window(1024, dtype=torch.float64)
    rows = torch.zeros((3 * T, 1032), dtype=torch.float32)
    clips = []
    for b, (kind, n) in enumerate(zip(("harmonic", "chirp", "noise"), lens)):
        x = synth.make_clip(kind, 256 * n, amplitude=0.1).double()
        spec = vr.stft_same(x, n, window)
        assert float(spec.abs().max()) < 100.0
        rows[b * T:b * T + n] = _head_rows(spec)
        clips.append(x)
    ml = torch.tensor(lens)
    audio, alen = _head(rows, T, ml)
    _check_padding(audio, alen, ml)
    for b, x in enumerate(clips):
        err = float((audio[b, :x.shape[0]].double() - x).abs().max())
        assert err <= 1e-5 * float(x.abs().max()), f"clip {b}: {err:.3e}"


def test_istft_head_clip_and_nan():
    """log-magnitudes above log(100) give magnitude exactly 100 (10 and 20 give the same bits, equal to mag 100 in float64);
    a NaN in a valid frame reaches exactly the samples that frame covers."""
    T = 12
    g = torch.Generator().manual_seed(5)
    h = torch.zeros((T, 1032))
    h[:, 513:1026] = torch.rand((T, 513), generator=g) * 600 - 300
    h_hi, h_hi2 = h.clone(), h.clone()
    h_hi[:, :513], h_hi2[:, :513] = 10.0, 20.0
    a1, _ = _head(h_hi, T, torch.tensor([T]))
    a2, _ = _head(h_hi2, T, torch.tensor([T]))
    assert torch.equal(a1, a2)
    head = vr.ISTFTHead(64).double()
    ref = head.spectrum_to_audio(h_hi[:, :1026].double().T[None])[0]
    assert float((a1[0, :256 * T].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())

    f = 5
    h_nan = h_hi.clone()
    h_nan[f, 3] = float("nan")
    a3, _ = _head(h_nan, T, torch.tensor([T]))
    lo, hi = max(0, 256 * f - 384), min(256 * T, 256 * f + 640)
    assert torch.isnan(a3[0, lo:hi]).all()
    assert torch.equal(a3[0, :lo], a1[0, :lo]) and torch.equal(a3[0, hi:], a1[0, hi:])


# ------------------------------------------------------------------------------------------------------------ padding
def test_padding_semantics(models):
    voc = models["official"][2]
    mel, ml = _mel("official", "ragged")
    ml_d = ml.to(DEV)
    base, alen = voc(mel.to(DEV), ml_d)
    # NaN past mel_len changes nothing
    noisy = mel.clone()
    for b in range(3):
        noisy[b, :, int(ml[b]):] = float("nan")
    a_nan, _ = voc(noisy.to(DEV), ml_d)
    assert torch.equal(a_nan, base)
    # other utterances' content leaves utterance 1 bit-identical
    other = mel.clone()
    other[0] += 3.0
    other[2] *= -1.0
    a_other, _ = voc(other.to(DEV), ml_d)
    assert torch.equal(a_other[1], base[1])
    _check_padding(base.cpu(), alen.cpu(), ml)
    # an utterance inside the batch equals it vocoded alone (to the fp32 bound)
    n = int(ml[1])
    alone, _ = voc(mel[1:2, :, :n].to(DEV))
    peak = float(alone.abs().max())
    assert float((alone[0] - base[1, :256 * n]).abs().max()) <= FP32_REL * peak
    # device lengths outside [0, T] give a zero row and audio_len 0
    T = mel.shape[2]
    bad = torch.tensor([-1, int(ml[1]), T + 1], dtype=torch.int64, device=DEV)
    a_bad, l_bad = voc(mel.to(DEV), bad)
    torch.cuda.synchronize()
    assert l_bad.tolist() == [0, 256 * int(ml[1]), 0]
    assert (a_bad[0] == 0).all() and (a_bad[2] == 0).all()
    assert torch.equal(a_bad[1], base[1])


# ------------------------------------------------------------------------------------------- determinism and capture
def test_determinism_and_graph_replay(models):
    voc = models["official"][2]
    mel, ml = _mel("official", "ragged")
    mel, ml = mel.to(DEV), ml.to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        voc.set_compute_dtype(dtype)
        try:
            a1, _ = voc(mel, ml)
            a2, _ = voc(mel, ml)
            assert torch.equal(a1, a2)
            out = voc.empty_outputs(mel.shape[0], mel.shape[2], DEV)
            g = graph.GraphedCall(lambda: voc(mel, ml, out=out))
            eager = a1.clone()
            out[0].zero_()
            audio, _ = g.replay()
            torch.cuda.synchronize()
            assert torch.equal(audio, eager)
        finally:
            voc.set_compute_dtype(torch.float32)


def test_text_to_waveform_as_one_graph(models):
    """AcousticModel.infer(..., max_dec_len) then the vocoder, captured as one HIP graph, equals the eager chain bit for bit."""
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    model = AcousticModel.init(AcousticDims().model_config()).eval()
    model.load_state_dict(synth.make_state_dict(), strict=True)
    model = model.to(DEV).requires_grad_(False)
    voc = models["official"][2]
    inp = synth.make_inputs(3, 40, 96, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 40), 2, dtype=torch.int64, device=DEV)
    out = voc.empty_outputs(3, 80, DEV)

    def chain():
        mel, ao = model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=80)
        return voc(mel, ao.dec_lengths, out=out)

    eager = [t.clone() for t in chain()]
    torch.cuda.synchronize()
    g = graph.GraphedCall(chain)
    out[0].zero_()
    audio, alen = g.replay()
    torch.cuda.synchronize()
    assert torch.equal(audio, eager[0]) and torch.equal(alen, eager[1])
    assert torch.isfinite(audio).all() and (alen > 0).all()


def test_vocoder_issues_no_aten_compute_ops(models):
    from torch.utils._python_dispatch import TorchDispatchMode
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream")
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not str(func).startswith(harmless):
                seen.append(str(func))
            return func(*args, **(kwargs or {}))

    voc = models["official"][2]
    mel, ml = _mel("official", "ragged")
    ml = ml.to(DEV)
    for m in (mel.to(DEV), mel.to(DEV).half()):
        for dtype in (torch.float32, torch.bfloat16):
            voc.set_compute_dtype(dtype)
            try:
                voc(m, ml)                      # stages the weight images outside the watched call
                torch.cuda.synchronize()
                with Watch():
                    voc(m, ml)
                    voc.infer(m)
                torch.cuda.synchronize()
            finally:
                voc.set_compute_dtype(torch.float32)
            assert not seen, f"{m.dtype} / {dtype}: PyTorch compute ops inside the vocoder: {sorted(set(seen))}"


def test_notebook_mel2audio_call(models):
    """The notebook's mel2audio body, unchanged, under autocast and inference_mode; an fp16 mel gives the audio of its fp32
    upcast bit for bit."""
    vocoder = models["official"][2]
    mel = synth.make_vocoder_mel(1, 80, 50).to(DEV)
    with torch.amp.autocast(device_type="cuda"), torch.inference_mode():
        audio = vocoder.infer(mel.half()).squeeze().cpu().numpy()
    assert audio.shape == (50 * 256,) and audio.dtype.name == "float32"
    up, _ = vocoder(mel.half().float())
    assert torch.equal(torch.from_numpy(audio), up[0].cpu())
    assert math.isfinite(float(abs(audio).max()))
