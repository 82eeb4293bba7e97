"""CPU: the vocoder's loader (plain dict, torch.save file, {"state_dict": ...}, a TorchScript archive in fp16 under an extra
prefix, no gamma), its refusals, its ISTFT tables, that CPU tensors raise, and that the float64 reference's ISTFT_same inverts
a same-framed STFT."""
import math

import numpy as np
import pytest
import torch

import vocos_reference as vr
from isp_tts_amd import runtime, synth
from isp_tts_amd.vocoder import Vocoder

SMALL = (100, 128, 256, 2)


def _sd(**kw):
    return synth.make_vocoder_state_dict(SMALL, **kw)


def _check_loaded(v: Vocoder, sd: dict, gamma: bool = True):
    assert (v.n_mels, v.dim, v.inter, v.num_layers, v.has_gamma) == (*SMALL, gamma)
    assert v.k_pad == 704
    own = v.state_dict()
    for k, t in own.items():
        assert t.dtype == torch.float32
        assert torch.equal(t, sd[k].float()), k
    Vocoder(*SMALL, gamma=gamma).load_state_dict(own, strict=True)


def test_load_plain_dict_and_files(tmp_path):
    sd = _sd()
    _check_loaded(Vocoder.from_state_dict(sd), sd)
    torch.save(sd, tmp_path / "plain.pt")
    _check_loaded(Vocoder.from_pretrained(tmp_path / "plain.pt"), sd)
    torch.save({"state_dict": sd, "epoch": 3}, tmp_path / "wrapped.ckpt")
    _check_loaded(Vocoder.from_pretrained(tmp_path / "wrapped.ckpt"), sd)


def test_load_torchscript_fp16_archive_under_a_prefix(tmp_path):
    sd = _sd()

    class Wrapper(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.vocos = vr.build(sd, torch.float32)

        def forward(self, mel):
            return self.vocos(mel)

    scripted = torch.jit.script(Wrapper().half())
    scripted.save(str(tmp_path / "vocos_fp16.pts"))
    v = Vocoder.from_pretrained(tmp_path / "vocos_fp16.pts")
    assert (v.n_mels, v.dim, v.inter, v.num_layers, v.has_gamma) == (*SMALL, True)
    for k, t in v.state_dict().items():
        assert t.dtype == torch.float32
        assert torch.equal(t, sd[k].half().float()), k


def test_load_without_gamma():
    sd = _sd(gamma=False)
    v = Vocoder.from_state_dict(sd)
    _check_loaded(v, sd, gamma=False)
    assert all(b.gamma is None for b in v.backbone.convnext)


def test_feature_extractor_keys_are_ignored():
    sd = _sd()
    sd["feature_extractor.mel_spec.spectrogram.window"] = torch.ones(1024)
    Vocoder.from_state_dict(sd)


@pytest.mark.parametrize("what, edit, exc, match", [
    ("adaln", lambda sd: sd.update({"backbone.convnext.0.norm.scale.weight": torch.ones(4, 128)}), NotImplementedError,
     "AdaLayerNorm"),
    ("n_fft", lambda sd: sd.update({"head.out.weight": torch.zeros(514, 128), "head.out.bias": torch.zeros(514)}),
     NotImplementedError, "n_fft"),
    ("window", lambda sd: sd.update({"head.istft.window": torch.ones(512)}), NotImplementedError, "n_fft"),
    ("dim", lambda sd: sd.update({"backbone.embed.weight": torch.zeros(96, 100, 7)}), NotImplementedError, "dim 96"),
    ("dim_big", lambda sd: sd.update({"backbone.embed.weight": torch.zeros(1088, 100, 7)}), NotImplementedError, "dim 1088"),
    ("inter", lambda sd: sd.update({"backbone.convnext.0.pwconv1.weight": torch.zeros(250, 128)}), NotImplementedError,
     "intermediate"),
    ("mels", lambda sd: sd.update({"backbone.embed.weight": torch.zeros(128, 129, 7)}), NotImplementedError, "n_mels"),
    ("missing", lambda sd: sd.pop("backbone.convnext.1.pwconv2.bias"), ValueError, "missing keys"),
    ("missing_embed", lambda sd: sd.pop("backbone.embed.weight"), ValueError, "missing keys"),
])
def test_refusals(what, edit, exc, match):
    sd = _sd()
    edit(sd)
    with pytest.raises(exc, match=match):
        Vocoder.from_state_dict(sd)


def test_refuses_other_hop_and_padding():
    sd = _sd()
    with pytest.raises(NotImplementedError, match="hop_length other than 256 is not built"):
        Vocoder.from_state_dict(sd, hop_length=320)
    with pytest.raises(NotImplementedError, match="same"):
        Vocoder.from_state_dict(sd, padding="center")
    with pytest.raises(NotImplementedError, match="fp32 and bf16"):
        Vocoder.from_state_dict(sd).set_compute_dtype(torch.float16)


def test_tables():
    v = Vocoder.from_state_dict(_sd())
    t = v.tables()
    assert t.dtype == torch.float32 and t.shape == (5120,)
    m = np.arange(2048)
    tw = t[:4096].view(2048, 2).double().numpy()
    assert np.abs(tw[:, 0] - np.cos(2 * np.pi * m / 2048)).max() < 6e-8
    assert np.abs(tw[:, 1] + np.sin(2 * np.pi * m / 2048)).max() < 6e-8
    assert torch.equal(t[4096:], torch.hann_window(1024, dtype=torch.float32))


def test_cpu_tensors_raise():
    v = Vocoder.from_state_dict(_sd())
    with pytest.raises(runtime.IspkError, match="GPU"):
        v(torch.zeros(1, 100, 4))
    with pytest.raises(runtime.IspkError, match="GPU"):
        v.infer(torch.zeros(1, 100, 4))


@pytest.mark.parametrize("T", [1, 2, 3, 7, 100])
def test_reference_istft_inverts_a_same_framed_stft(T):
    x = torch.from_numpy(np.random.default_rng(T).standard_normal(256 * T))
    istft = vr.ISTFT().double()
    y = istft(vr.stft_same(x, T, istft.window)[None])[0]
    assert y.shape == x.shape
    assert float((y - x).abs().max()) <= 1e-12


def test_reference_envelope_minimum():
    """The envelope near the ends depends on T: min 0.7286 for T = 1, 0.75 for T >= 2; 1.5 inside."""
    w2 = torch.hann_window(1024, dtype=torch.float64) ** 2
    for T, lo in ((1, 0.7286), (2, 0.75), (9, 0.75)):
        env = torch.zeros((T - 1) * 256 + 1024, dtype=torch.float64)
        for t in range(T):
            env[256 * t:256 * t + 1024] += w2
        env = env[384:384 + 256 * T]
        assert math.isclose(float(env.min()), lo, abs_tol=5e-5)
    assert math.isclose(float(env[1024:-1024].max()), 1.5, abs_tol=1e-12)
