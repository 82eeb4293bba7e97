"""CPU: the HiFi-GAN generator's construction and loader (three weight-norm forms, key prefixes, the {"generator": ...} wrapper,
config from a dict / a path / a config.json beside the checkpoint / the official defaults), its refusals, hop_length, that CPU
tensors raise, and the argument checks of the new C entries, which run before any launch."""
import ctypes
import json

import pytest
import torch

import hifigan_reference as hr
from isp_tts_amd import runtime, synth
from isp_tts_amd.hifigan import CONFIGS, HifiGan

DIMS = synth.HIFIGAN_DIMS
E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4


@pytest.mark.parametrize("name, hop", [("v1", 256), ("v3", 256), ("odd", 6)])
def test_construct_and_hop_length(name, hop):
    m = HifiGan(**DIMS[name])
    assert m.hop_length == hop
    sd = synth.make_hifigan_state_dict(DIMS[name])
    assert sorted(m.state_dict()) == sorted(sd)
    m.load_state_dict(sd, strict=True)                      # the official names, plain weight / bias
    audio, alen = m.empty_outputs(3, 5, "cpu")
    assert audio.shape == (3, 5 * hop) and alen.dtype == torch.int64
    assert CONFIGS["v1"] == DIMS["v1"] and CONFIGS["v3"] == DIMS["v3"]


@pytest.mark.parametrize("name", ["v3", "odd"])
def test_weight_norm_forms_fold_to_the_same_weights(name):
    cfg = DIMS[name]
    plain = synth.make_hifigan_state_dict(cfg)
    for form in ("g_v", "parametrized"):
        sd = synth.make_hifigan_state_dict(cfg, weight_norm=form)
        suffix = ".weight_v" if form == "g_v" else ".parametrizations.weight.original1"
        g_suffix = ".weight_g" if form == "g_v" else ".parametrizations.weight.original0"
        assert not any(k.endswith(".weight") for k in sd)
        v = sd["ups.0" + suffix]
        assert sd["ups.0" + g_suffix].shape == (v.shape[0], 1, 1)                     # C_in axis of a ConvTranspose1d
        assert not torch.allclose(sd["ups.0" + g_suffix].flatten(), v.flatten(1).norm(dim=1), rtol=0.05)   # g != ||v||
        ref = hr.fold(sd)
        got = HifiGan.from_state_dict(sd, cfg).state_dict()
        assert sorted(got) == sorted(plain)
        for k, t in got.items():
            assert t.dtype == torch.float32
            scale = float(ref[k].abs().max())
            assert float((t.double() - ref[k]).abs().max()) <= 1e-6 * scale, k        # the reference's own float64 folding
            assert float((t - plain[k]).abs().max()) <= 1e-6 * scale, k               # = the plain weights
    # the norm runs over the C_in slices of the transposed convolution (dim 0 of [C_in, C_out, k]), not over C_out
    sd = synth.make_hifigan_state_dict(cfg, weight_norm="g_v")
    w = HifiGan.from_state_dict(sd, cfg).state_dict()["ups.0.weight"].double()
    g = sd["ups.0.weight_g"].double().flatten()
    assert w.shape[0] != w.shape[1]
    assert float((w.flatten(1).norm(dim=1) - g).abs().max()) <= 1e-6 * float(g.max())


def test_prefixes_wrappers_and_files(tmp_path):
    cfg = DIMS["odd"]
    sd = synth.make_hifigan_state_dict(cfg, weight_norm="g_v")
    want = HifiGan.from_state_dict(sd, cfg).state_dict()

    def same(m):
        assert all(torch.equal(t, want[k]) for k, t in m.state_dict().items())

    same(HifiGan.from_state_dict({"generator": sd}, cfg))
    same(HifiGan.from_state_dict({"state_dict": sd}, cfg))
    pre = {"model.vocoder.generator." + k: v for k, v in sd.items()}
    pre["model.mel.window"] = torch.ones(4)
    same(HifiGan.from_state_dict(pre, cfg))
    torch.save({"generator": sd}, tmp_path / "g_odd")
    same(HifiGan.from_pretrained(tmp_path / "g_odd", cfg))
    torch.save(sd, tmp_path / "bare.pt")
    same(HifiGan.from_pretrained(tmp_path / "bare.pt", cfg))


def test_config_from_dict_path_beside_and_defaults(tmp_path):
    # strides and dilations cannot be read from the weights: other values than the defaults must come through
    cfg = dict(DIMS["odd"], upsample_rates=(5, 2), resblock_dilation_sizes=((1, 2, 4), (1, 1, 1)))
    sd = synth.make_hifigan_state_dict(cfg)
    m = HifiGan.from_state_dict(sd, cfg)
    assert m.rates == (5, 2) and m.res_dilations == ((1, 2, 4), (1, 1, 1)) and m.hop_length == 10
    official = {"resblock": "1", "num_mels": 20, "upsample_rates": [5, 2], "upsample_kernel_sizes": [7, 4],
                "upsample_initial_channel": 128, "resblock_kernel_sizes": [3, 11],
                "resblock_dilation_sizes": [[1, 2, 4], [1, 1, 1]], "sampling_rate": 22050}
    (tmp_path / "elsewhere").mkdir()
    path = tmp_path / "elsewhere" / "cfg.json"
    path.write_text(json.dumps(official))
    assert HifiGan.from_state_dict(sd, path).config() == m.config()
    torch.save({"generator": sd}, tmp_path / "g_0001")
    assert HifiGan.from_pretrained(tmp_path / "g_0001").rates == (3, 2)              # no config: stride = kernel // 2
    assert HifiGan.from_pretrained(tmp_path / "g_0001", str(path)).rates == (5, 2)
    (tmp_path / "config.json").write_text(json.dumps(official))
    assert HifiGan.from_pretrained(tmp_path / "g_0001").config() == m.config()       # config.json beside the checkpoint
    # the official defaults
    for name in ("v3", "odd"):
        d = HifiGan.from_state_dict(synth.make_hifigan_state_dict(DIMS[name]))
        assert d.config() == {k: v for k, v in HifiGan(**DIMS[name]).config().items()}
    with pytest.raises(ValueError, match="does not fit"):
        HifiGan.from_state_dict(sd, dict(cfg, upsample_rates=(3, 2, 2)))
    with pytest.raises(ValueError, match="does not fit"):
        HifiGan.from_state_dict(sd, dict(cfg, resblock_kernel_sizes=(3, 7)))


def test_error_classes():
    cfg = DIMS["odd"]
    sd = synth.make_hifigan_state_dict(cfg)
    for drop in ("resblocks.1.convs2.2.bias", "conv_pre.weight", "ups.1.weight", "conv_post.bias"):
        bad = {k: v for k, v in sd.items() if k != drop}
        with pytest.raises(ValueError, match="missing keys"):
            HifiGan.from_state_dict(bad, cfg)
    bad = {k.replace("resblocks.3.", "resblocks.7."): v for k, v in sd.items()}      # misnumbered
    with pytest.raises(ValueError, match="missing keys"):
        HifiGan.from_state_dict(bad, cfg)
    gv = synth.make_hifigan_state_dict(cfg, weight_norm="g_v")
    gv.pop("ups.0.weight_g")
    with pytest.raises(ValueError, match="missing keys"):
        HifiGan.from_state_dict(gv, cfg)
    with pytest.raises(NotImplementedError, match="channel count 16"):              # V2 ends at 16 and 8 channels
        HifiGan(**CONFIGS["v2"])
    with pytest.raises(NotImplementedError, match="channel count 1024"):
        HifiGan(**dict(cfg, upsample_initial_channel=1024))
    with pytest.raises(NotImplementedError, match="k - stride even"):
        HifiGan(**dict(cfg, upsample_kernel_sizes=(8, 4)))
    with pytest.raises(NotImplementedError, match="k >= stride"):
        HifiGan(**dict(cfg, upsample_rates=(3, 6)))
    with pytest.raises(NotImplementedError, match="resblock kernel 4"):
        HifiGan(**dict(cfg, resblock_kernel_sizes=(3, 4)))
    with pytest.raises(NotImplementedError, match="dilation 13"):
        HifiGan(**dict(cfg, resblock_dilation_sizes=((1, 3, 13), (1, 3, 5))))
    with pytest.raises(NotImplementedError, match="n_mels"):
        HifiGan(**dict(cfg, n_mels=129))
    with pytest.raises(NotImplementedError, match="fp32 and bf16"):
        HifiGan(**cfg).set_compute_dtype(torch.float16)
    m = HifiGan(**cfg)
    with pytest.raises(runtime.IspkError, match="GPU"):
        m(torch.zeros(1, 20, 4))
    with pytest.raises(runtime.IspkError, match="GPU"):
        m.infer(torch.zeros(1, 20, 4))
    x = torch.zeros(8, 32)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.hifigan_conv(x, 8, torch.zeros(3, 32, 32), None, 3)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.hifigan_upsample(x, 8, torch.zeros(4, 32, 32), None, 4, 2)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.hifigan_post(x, 8, torch.zeros(7, 32), torch.zeros(1), torch.zeros(1, 8))


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    assert lib.ispk_hifigan_tile_rows() == runtime.HIFIGAN_TILE_ROWS
    one = ctypes.c_void_p(16)      # never dereferenced: the checks fail first
    err = lambda: lib.ispk_last_error_string()
    for conv in (lib.ispk_hifigan_conv_f32, lib.ispk_hifigan_conv_bf16):
        args = lambda **kw: tuple({**dict(x=one, ldx=64, w=one, bias=None, resid=None, ldr=0, out=one, ldo=64, len=None,
                                          len_mul=1, B=2, T=9, C_in=64, C_out=64, k=3, d=1, slope=0.1, scale=1.0, acc=0,
                                          stream=None), **kw}.values())
        assert conv(*args(x=None)) == E_NULL and b"null" in err()
        assert conv(*args(w=None)) == E_NULL
        assert conv(*args(out=None)) == E_NULL
        assert conv(*args(k=4)) == E_UNSUP and b"odd k" in err()
        assert conv(*args(k=13)) == E_UNSUP
        assert conv(*args(d=13)) == E_UNSUP and b"dilation" in err()
        assert conv(*args(C_in=48, ldx=48)) == E_UNSUP and b"channel count" in err()
        assert conv(*args(C_out=16, ldo=16)) == E_UNSUP
        assert conv(*args(C_in=544, ldx=544)) == E_UNSUP
        assert conv(*args(ldx=32)) == E_SHAPE
        assert conv(*args(ldo=66)) == E_ALIGN
        assert conv(*args(x=ctypes.c_void_p(20))) == E_ALIGN
        assert conv(*args(B=70000)) == E_SHAPE
        assert conv(*args(B=0, x=None)) == 0 and conv(*args(T=0, x=None)) == 0          # zero-sized: no-ops
    for up in (lib.ispk_hifigan_upsample_f32, lib.ispk_hifigan_upsample_bf16):
        args = lambda **kw: tuple({**dict(x=one, ldx=64, w=one, bias=None, out=one, ldo=32, len=None, len_mul=1, B=2, T=9,
                                          C_in=64, C_out=32, k=16, u=8, slope=0.1, stream=None), **kw}.values())
        assert up(*args(out=None)) == E_NULL and b"null" in err()
        assert up(*args(k=7, u=2)) == E_UNSUP and b"even" in err()                      # k - stride odd
        assert up(*args(k=4, u=8)) == E_UNSUP                                           # k < stride
        assert up(*args(C_out=8, ldo=8)) == E_UNSUP and b"channel count" in err()
        assert up(*args(T=2 ** 30)) == E_SHAPE
        assert up(*args(B=0, x=None)) == 0 and up(*args(T=0, x=None)) == 0
    post = lib.ispk_hifigan_post_f32
    args = lambda **kw: tuple({**dict(x=one, ldx=32, w=one, bias=one, len=None, len_mul=1, audio=one, lda=9, alen=None, B=2,
                                      T=9, S=9, C=32, slope=0.01, stream=None), **kw}.values())
    assert post(*args(audio=None)) == E_NULL and b"null" in err()
    assert post(*args(w=None)) == E_NULL
    assert post(*args(C=8, ldx=8)) == E_UNSUP and b"channel count" in err()
    assert post(*args(S=8)) == E_SHAPE
    assert post(*args(lda=8)) == E_SHAPE
    assert post(*args(ldx=34)) == E_ALIGN
    assert post(*args(B=0, audio=None)) == 0
