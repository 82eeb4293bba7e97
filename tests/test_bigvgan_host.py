"""CPU: the BigVGAN generator's construction and loader (three weight-norm forms, key prefixes, the {"generator": ...}
wrapper, geometry and flags from names and config, conv_post without a bias), its refusals, the anti-aliasing taps, that CPU
tensors raise, and the argument checks of ispk_snake_aa_f32 and ispk_hifigan_post_clamp_f32, which run before any launch."""
import ctypes
import json
import math

import pytest
import torch

import bigvgan_reference as br
from isp_tts_amd import runtime, synth
from isp_tts_amd.bigvgan import BigVGan, kaiser_sinc_filter

DIMS = synth.BIGVGAN_DIMS
E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4


@pytest.mark.parametrize("name, hop", [("base", 256), ("odd", 6), ("odd2", 6)])
def test_construct_and_hop_length(name, hop):
    m = BigVGan(**DIMS[name])
    assert m.hop_length == hop and m.config() == DIMS[name]
    sd = synth.make_bigvgan_state_dict(DIMS[name])
    assert sorted(m.state_dict()) == sorted(sd)
    m.load_state_dict(sd, strict=True)                      # the official names, plain weight / bias, filters as buffers
    assert ("conv_post.bias" in sd) == DIMS[name]["use_bias_at_final"]
    assert ("activation_post.act.beta" in sd) == (DIMS[name]["activation"] == "snakebeta")
    assert "ups.0.0.weight" in sd and "resblocks.0.activations.0.upsample.filter" in sd
    assert "resblocks.0.activations.0.downsample.lowpass.filter" in sd and sd["activation_post.upsample.filter"].shape == (1, 1, 12)
    n_act = sum(k.endswith(".act.alpha") for k in sd)
    per_block = sum(len(D) for D in DIMS[name]["resblock_dilation_sizes"]) * (2 if DIMS[name]["resblock"] == "1" else 1)
    assert n_act == len(DIMS[name]["upsample_rates"]) * per_block + 1
    audio, alen = m.empty_outputs(3, 5, "cpu")
    assert audio.shape == (3, 5 * hop) and alen.dtype == torch.int64


def test_taps_are_the_kaiser_sinc_filter():
    A = 2.285 * 5 * math.pi * 1.2 + 7.95
    beta_k = 0.1102 * (A - 8.7)
    j = torch.arange(12, dtype=torch.float64)
    f = 0.5 * torch.kaiser_window(12, periodic=False, beta=beta_k, dtype=torch.float64) * torch.sinc(0.5 * (j - 5.5))
    f = f / f.sum()
    assert abs(float(f[0]) - 0.0020290) < 5e-8 and abs(float(f[5]) - 0.4432098) < 5e-8 and float(f[5]) == float(f[6])
    assert float((kaiser_sinc_filter() - f).abs().max()) <= 1e-12
    assert float((br.kaiser_sinc_taps() - f).abs().max()) <= 1e-12
    assert float((synth.bigvgan_filter() - f).abs().max()) <= 1e-12
    m = BigVGan(**DIMS["odd"])                               # built from a config alone: the formula, in fp32
    for name, buf in m.named_buffers():
        assert name.endswith(".filter") and buf.shape == (1, 1, 12) and torch.equal(buf.flatten(), f.float()), name
    loaded = BigVGan.from_state_dict(synth.make_bigvgan_state_dict(DIMS["odd"]), DIMS["odd"])
    assert all(torch.equal(b, dict(m.named_buffers())[n]) for n, b in loaded.named_buffers())
    # the taps in a checkpoint rule
    sd = synth.make_bigvgan_state_dict(DIMS["odd"])
    sd["resblocks.1.activations.2.upsample.filter"] = torch.arange(12.0).reshape(1, 1, 12)
    got = BigVGan.from_state_dict(sd, DIMS["odd"])
    assert torch.equal(got.resblocks[1].activations[2].upsample.filter.flatten(), torch.arange(12.0))
    assert torch.equal(got.staged()["blocks"][1][1][0][0][2][:12], torch.arange(12.0))


@pytest.mark.parametrize("name", ["odd", "odd2"])
def test_weight_norm_forms_fold_to_the_same_weights(name):
    cfg = DIMS[name]
    plain = synth.make_bigvgan_state_dict(cfg)
    for form in ("g_v", "parametrized"):
        sd = synth.make_bigvgan_state_dict(cfg, weight_norm=form)
        suffix = ".weight_v" if form == "g_v" else ".parametrizations.weight.original1"
        g_suffix = ".weight_g" if form == "g_v" else ".parametrizations.weight.original0"
        assert not any(k.endswith(".weight") for k in sd)
        v = sd["ups.0.0" + suffix]
        assert sd["ups.0.0" + g_suffix].shape == (v.shape[0], 1, 1)                   # C_in axis of a ConvTranspose1d
        assert not torch.allclose(sd["ups.0.0" + g_suffix].flatten(), v.flatten(1).norm(dim=1), rtol=0.05)   # g != ||v||
        ref = br.fold(sd)
        got = BigVGan.from_state_dict(sd, cfg).state_dict()
        assert sorted(got) == sorted(plain)
        for k, t in got.items():
            assert t.dtype == torch.float32
            scale = float(ref[k].abs().max())
            assert float((t.double() - ref[k]).abs().max()) <= 1e-6 * scale, k        # the reference's own float64 folding
            assert float((t - plain[k]).abs().max()) <= 1e-6 * scale, k               # = the plain weights


def test_prefixes_wrappers_and_files(tmp_path):
    cfg = DIMS["odd"]
    sd = synth.make_bigvgan_state_dict(cfg, weight_norm="g_v")
    want = BigVGan.from_state_dict(sd, cfg).state_dict()

    def same(m):
        assert all(torch.equal(t, want[k]) for k, t in m.state_dict().items())

    same(BigVGan.from_state_dict({"generator": sd}, cfg))
    same(BigVGan.from_state_dict({"state_dict": sd}, cfg))
    pre = {"model.vocoder.generator." + k: v for k, v in sd.items()}
    pre["model.mel.window"] = torch.ones(4)
    same(BigVGan.from_state_dict(pre, cfg))
    torch.save({"generator": sd}, tmp_path / "bigvgan_generator.pt")
    same(BigVGan.from_pretrained(tmp_path / "bigvgan_generator.pt", cfg))
    torch.save(sd, tmp_path / "bare.pt")
    same(BigVGan.from_pretrained(tmp_path / "bare.pt", cfg))


def test_geometry_and_flags_from_names_and_config(tmp_path):
    # read from shapes and names: C0, n_mels, up-kernels, block type, block kernels, snake / snakebeta
    for name in ("base", "odd", "odd2"):
        cfg = DIMS[name]
        m = BigVGan.from_state_dict(synth.make_bigvgan_state_dict(cfg), cfg)
        assert m.config() == cfg
    flags = dict(snake_logscale=False, use_bias_at_final=False, use_tanh_at_final=False)
    none = BigVGan.from_state_dict(synth.make_bigvgan_state_dict(DIMS["odd"]), {k: DIMS["odd"][k] for k in flags})
    assert none.config() == dict(DIMS["odd"], upsample_rates=(3, 2))                  # stride = kernel // 2, dilations (1, 3, 5)
    # the published defaults: snakebeta (from act.beta), logscale, bias, tanh
    d = BigVGan.from_state_dict(synth.make_bigvgan_state_dict(DIMS["base"]))
    assert d.config() == DIMS["base"]
    # strides, dilations and the three flags cannot be read from the weights: other values must come through
    cfg = dict(DIMS["odd2"], upsample_rates=(5, 2), resblock_dilation_sizes=((1, 2), (4, 1)), snake_logscale=True,
               use_tanh_at_final=True)
    sd = synth.make_bigvgan_state_dict(cfg)
    m = BigVGan.from_state_dict(sd, cfg)
    assert m.rates == (5, 2) and m.res_dilations == ((1, 2), (4, 1)) and m.hop_length == 10 and m.resblock == "2"
    assert m.snake_logscale and m.use_tanh_at_final and not m.use_bias_at_final and m.activation == "snake"
    official = {"resblock": "2", "num_mels": 20, "upsample_rates": [5, 2], "upsample_kernel_sizes": [7, 4],
                "upsample_initial_channel": 128, "resblock_kernel_sizes": [3, 11], "resblock_dilation_sizes": [[1, 2], [4, 1]],
                "activation": "snake", "snake_logscale": True, "use_bias_at_final": False, "use_tanh_at_final": True,
                "use_cuda_kernel": True, "sampling_rate": 22050}
    (tmp_path / "elsewhere").mkdir()
    path = tmp_path / "elsewhere" / "cfg.json"
    path.write_text(json.dumps(official))
    assert BigVGan.from_state_dict(sd, path).config() == m.config()                  # use_cuda_kernel is ignored
    torch.save({"generator": sd}, tmp_path / "g.pt")
    assert BigVGan.from_pretrained(tmp_path / "g.pt", str(path)).config() == m.config()
    (tmp_path / "config.json").write_text(json.dumps(official))
    assert BigVGan.from_pretrained(tmp_path / "g.pt").config() == m.config()          # config.json beside the checkpoint
    # a config that contradicts the weights
    with pytest.raises(ValueError, match="does not fit"):
        BigVGan.from_state_dict(sd, dict(cfg, upsample_rates=(3, 2, 2)))
    with pytest.raises(ValueError, match="does not fit"):
        BigVGan.from_state_dict(sd, dict(cfg, resblock_kernel_sizes=(3, 7)))
    with pytest.raises(ValueError, match="does not fit.*resblock '1'"):
        BigVGan.from_state_dict(sd, dict(cfg, resblock="1"))
    with pytest.raises(ValueError, match="does not fit.*activation 'snakebeta'"):
        BigVGan.from_state_dict(sd, dict(cfg, activation="snakebeta"))


def test_conv_post_bias_and_use_bias_at_final():
    cfg = DIMS["odd"]
    sd = synth.make_bigvgan_state_dict(cfg)
    assert "conv_post.bias" not in sd
    m = BigVGan.from_state_dict(sd, cfg)
    assert m.conv_post.bias is None and torch.equal(m.staged()["post_b"], torch.zeros(1))   # a staged zero
    with pytest.raises(ValueError, match=r"missing keys.*conv_post\.bias"):
        BigVGan.from_state_dict(sd, dict(cfg, use_bias_at_final=True))
    with pytest.raises(ValueError, match=r"missing keys.*conv_post\.bias"):          # true is the default
        BigVGan.from_state_dict(sd, {k: v for k, v in cfg.items() if k != "use_bias_at_final"})
    with_bias = dict(sd, **{"conv_post.bias": torch.tensor([0.25])})
    assert float(BigVGan.from_state_dict(with_bias, dict(cfg, use_bias_at_final=True)).staged()["post_b"]) == 0.25
    with pytest.raises(ValueError, match="does not fit.*use_bias_at_final"):
        BigVGan.from_state_dict(with_bias, cfg)


def test_staged_activation_tables():
    """al and inv_b: float64, rounded once."""
    for name in ("base", "odd"):
        cfg = DIMS[name]
        sd = synth.make_bigvgan_state_dict(cfg)
        m = BigVGan.from_state_dict(sd, cfg)
        al, inv_b, taps = m.staged()["post_act"]
        a = sd["activation_post.act.alpha"].double()
        if cfg["snake_logscale"]:
            want_al, want_b = a.exp(), sd["activation_post.act.beta"].double().exp()
        else:
            want_al = want_b = a
        assert torch.equal(al, want_al.float()) and torch.equal(inv_b, (1.0 / (want_b + 1e-9)).float())
        assert al.dtype == inv_b.dtype == taps.dtype == torch.float32 and taps.shape == (24,)
        assert float(al.min()) >= 0.999 and float(al.max()) <= 6.001
        assert torch.equal(taps, torch.cat([synth.bigvgan_filter().float()] * 2))


def test_error_classes():
    cfg = DIMS["odd"]
    sd = synth.make_bigvgan_state_dict(cfg)
    for drop in ("resblocks.1.convs2.2.bias", "conv_pre.weight", "ups.1.0.weight", "resblocks.2.activations.3.act.alpha",
                 "activation_post.act.alpha", "resblocks.0.activations.0.downsample.lowpass.filter"):
        bad = {k: v for k, v in sd.items() if k != drop}
        with pytest.raises(ValueError, match="missing keys"):
            BigVGan.from_state_dict(bad, cfg)
    gv = synth.make_bigvgan_state_dict(cfg, weight_norm="g_v")
    gv.pop("ups.0.0.weight_g")
    with pytest.raises(ValueError, match="missing keys"):
        BigVGan.from_state_dict(gv, cfg)
    # the 112M models start at 1536 channels
    with pytest.raises(NotImplementedError, match="channel count 1536"):
        BigVGan(**dict(DIMS["base"], upsample_initial_channel=1536))
    with pytest.raises(NotImplementedError, match="channel count 16"):
        BigVGan(**dict(cfg, upsample_initial_channel=64))
    with pytest.raises(NotImplementedError, match="filter of 8 taps"):
        BigVGan(**dict(cfg, filter_size=8))
    bad = dict(sd, **{"activation_post.upsample.filter": torch.ones(1, 1, 16)})
    with pytest.raises(NotImplementedError, match="filter of 16 taps"):
        BigVGan.from_state_dict(bad, cfg)
    with pytest.raises(NotImplementedError, match="ratio 4 / 2"):
        BigVGan(**dict(cfg, up_ratio=4))
    with pytest.raises(NotImplementedError, match="ratio 2 / 3"):
        BigVGan.from_state_dict(sd, dict(cfg, down_ratio=3))
    with pytest.raises(NotImplementedError, match="activation 'gelu'"):
        BigVGan(**dict(cfg, activation="gelu"))
    with pytest.raises(NotImplementedError, match="k - stride even"):
        BigVGan(**dict(cfg, upsample_kernel_sizes=(8, 4)))
    with pytest.raises(NotImplementedError, match="fp32 and bf16"):
        BigVGan(**cfg).set_compute_dtype(torch.float16)
    m = BigVGan(**cfg)
    with pytest.raises(runtime.IspkError, match="GPU"):
        m(torch.zeros(1, 20, 4))
    with pytest.raises(runtime.IspkError, match="GPU"):
        m.infer(torch.zeros(1, 20, 4))
    x = torch.zeros(8, 32)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.snake_aa(x, 8, torch.zeros(32), torch.zeros(32), torch.zeros(24))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.hifigan_post(x, 8, torch.zeros(7, 32), torch.zeros(1), torch.zeros(1, 8), final_clamp=True)


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    assert lib.ispk_snake_aa_tile_rows() == runtime.SNAKE_AA_TILE_ROWS
    one, other = ctypes.c_void_p(16), ctypes.c_void_p(32)      # never dereferenced: the checks fail first
    err = lambda: lib.ispk_last_error_string()
    snake = lib.ispk_snake_aa_f32
    args = lambda **kw: tuple({**dict(x=one, ldx=64, al=one, inv_b=one, taps=one, out=other, ldo=64, len=None, len_mul=1, B=2,
                                      T=9, C=64, stream=None), **kw}.values())
    for name in ("x", "al", "inv_b", "taps", "out"):
        assert snake(*args(**{name: None})) == E_NULL and b"null" in err()
    assert snake(*args(C=48, ldx=48, ldo=48)) == E_UNSUP and b"channel count" in err()
    assert snake(*args(C=16, ldx=16, ldo=16)) == E_UNSUP
    assert snake(*args(C=544, ldx=544, ldo=544)) == E_UNSUP
    assert snake(*args(ldx=32)) == E_SHAPE and snake(*args(ldo=32)) == E_SHAPE
    assert snake(*args(ldo=66)) == E_ALIGN
    assert snake(*args(x=ctypes.c_void_p(20))) == E_ALIGN
    assert snake(*args(B=70000)) == E_SHAPE and snake(*args(len_mul=0)) == E_SHAPE
    assert snake(*args(out=one)) == E_SHAPE and b"may not be x" in err()               # out of place only
    assert snake(*args(B=0, x=None)) == 0 and snake(*args(T=0, x=None)) == 0           # zero-sized: no-ops
    post = lib.ispk_hifigan_post_clamp_f32
    args = lambda **kw: tuple({**dict(x=one, ldx=32, w=one, bias=one, len=None, len_mul=1, audio=one, lda=9, alen=None, B=2,
                                      T=9, S=9, C=32, slope=1.0, stream=None), **kw}.values())
    assert post(*args(audio=None)) == E_NULL and b"ispk_hifigan_post_clamp_f32: null" in err()
    assert post(*args(w=None)) == E_NULL
    assert post(*args(C=8, ldx=8)) == E_UNSUP and b"channel count" in err()
    assert post(*args(S=8)) == E_SHAPE
    assert post(*args(lda=8)) == E_SHAPE
    assert post(*args(ldx=34)) == E_ALIGN
    assert post(*args(B=0, audio=None)) == 0
