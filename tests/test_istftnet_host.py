"""CPU: the iSTFTNet generator's float64 reference (its torch.istft against a literal numpy restatement), construction and
loader (geometry from shapes, n_fft from conv_post, three weight-norm forms, a key prefix, a config.json beside the file, the
mismatch errors, the refusals), that the GPU tests' inputs are informative, that the synthetic HiFi-GAN / BigVGAN weights are
what they were before `_make_generator` got `post_channels`, and the argument checks of the new C entry."""
import ctypes
import hashlib
import json
import math

import numpy as np
import pytest
import torch

import istftnet_reference as ir
from isp_tts_amd import runtime, synth
from isp_tts_amd.istftnet import CONFIGS, IstftNet

DIMS = synth.ISTFTNET_DIMS
E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4
# name -> (B, T, lengths or None, strided): tests/test_gpu_hifigan.py's cases, which tests/test_gpu_istftnet.py runs
CASES = {"b1_t1": (1, 1, None, False), "b1_t2": (1, 2, None, False), "ragged": (3, 43, [1, 7, 43], False),
         "zero_len": (4, 17, [5, 0, 17, 9], False), "strided": (2, 12, [12, 9], True), "no_len": (2, 5, None, False)}


# --------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("n_fft, hop", [(16, 4), (8, 2), (20, 5)])
def test_reference_istft_equals_the_literal_sum(n_fft, hop):
    """torch.istft as the reference calls it = inverse DFT sum, Hann, overlap-add, / sum w^2, trim n_fft / 2, to float64
    rounding; and the imaginary parts of the DC and Nyquist bins do not matter."""
    g = torch.Generator().manual_seed(n_fft)
    H = n_fft // 2
    for frames in (3, 4, 5, 12):
        y = torch.randn((2, n_fft + 2, frames), generator=g, dtype=torch.float64)
        y[:, H + 1:] *= 3.0
        for ps in (1.0, math.pi):
            got = ir.head(y, n_fft, hop, ps)
            assert got.shape == (2, hop * (frames - 1))
            for b in range(2):
                spec = (torch.exp(y[b, :H + 1]) * torch.exp(1j * (ps * torch.sin(y[b, H + 1:])))).numpy()
                want = ir.istft_literal(spec, n_fft, hop)
                assert np.abs(got[b].numpy() - want).max() <= 1e-13 * np.abs(want).max()
                real_edges = spec.copy()
                real_edges[0], real_edges[H] = spec[0].real, spec[H].real          # DC and Nyquist: imaginary parts dropped
                assert np.abs(ir.istft_literal(real_edges, n_fft, hop) - want).max() <= 1e-13 * np.abs(want).max()
                assert np.abs(spec[0].imag).max() > 0.1 and np.abs(spec[H].imag).max() > 0.1


def test_reference_post_pads_one_frame_in_front():
    """R rows give R + 1 frames and hop R samples; frame 0 is row 1 (the reflection), frame i is row i - 1."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((1, 4, 6), generator=g, dtype=torch.float64)
    w = torch.randn((18, 4, 7), generator=g, dtype=torch.float64) * 0.1
    b = torch.randn((18,), generator=g, dtype=torch.float64) * 0.1
    audio, y = ir.post(x, w, b, 16, 4, want_y=True)
    assert audio.shape == (1, 24) and y.shape == (1, 18, 7)
    p = torch.cat([x[:, :, 1:2], x], dim=2)
    assert torch.equal(y, torch.nn.functional.conv1d(torch.nn.functional.leaky_relu(p, 0.01), w, b, padding=3))


def test_table():
    for n_fft in runtime.ISTFTNET_N_FFTS:
        t = runtime.istftnet_table(n_fft)
        assert t.shape == (4 * n_fft,) and t.dtype == torch.float32
        m = np.arange(n_fft)
        win = 0.5 - 0.5 * np.cos(2 * np.pi * m / n_fft)
        want = np.concatenate([np.cos(2 * np.pi * m / n_fft), np.sin(2 * np.pi * m / n_fft), win / n_fft, win * win])
        assert np.abs(t.double().numpy() - want).max() <= 2.0 ** -24


# ------------------------------------------------------------------------------------------- construction and loader
@pytest.mark.parametrize("name, hop", [("c8c8i", 256), ("odd", 12), ("n20", 30)])
def test_construct_and_hop_length(name, hop):
    m = IstftNet(**DIMS[name])
    assert m.hop_length == hop and m.conv_post.out_channels == DIMS[name]["gen_istft_n_fft"] + 2
    sd = synth.make_istftnet_state_dict(DIMS[name])
    assert sorted(m.state_dict()) == sorted(sd)
    m.load_state_dict(sd, strict=True)
    audio, alen = m.empty_outputs(3, 5, "cpu")
    assert audio.shape == (3, 5 * hop) and alen.dtype == torch.int64
    assert CONFIGS["c8c8i"] == DIMS["c8c8i"] and IstftNet().config() == dict(CONFIGS["c8c8i"], phase_scale=1.0)
    assert IstftNet.SLOPE == 0.1 and IstftNet.CONV_READS_STAGE is True


def test_loader_reads_the_geometry_from_shapes_and_config(tmp_path):
    for name in DIMS:
        cfg = DIMS[name]
        sd = synth.make_istftnet_state_dict(cfg)
        m = IstftNet.from_state_dict(sd, cfg)
        assert m.config() == IstftNet(**cfg).config()
        assert m.n_fft == cfg["gen_istft_n_fft"] and m.istft_hop == cfg["gen_istft_hop_size"]
    # without a config: n_fft from conv_post, hop n_fft / 4, stride = kernel / 2, phase_scale 1
    sd = synth.make_istftnet_state_dict(DIMS["c8c8i"])
    m = IstftNet.from_state_dict(sd)
    assert m.config() == IstftNet().config() and m.hop_length == 256
    n20 = IstftNet.from_state_dict(synth.make_istftnet_state_dict(DIMS["n20"]), {"resblock_dilation_sizes": ((1, 2), (2, 6))})
    assert (n20.n_fft, n20.istft_hop, n20.phase_scale, n20.resblock) == (20, 5, 1.0, "2")
    # the three weight-norm forms fold to the plain weights
    cfg = DIMS["odd"]
    plain = synth.make_istftnet_state_dict(cfg)
    for form in ("g_v", "parametrized"):
        sdw = synth.make_istftnet_state_dict(cfg, weight_norm=form)
        assert not any(k.endswith(".weight") for k in sdw)
        got = IstftNet.from_state_dict(sdw, cfg).state_dict()
        ref = ir.fold(sdw)
        assert sorted(got) == sorted(plain)
        for k, t in got.items():
            scale = float(ref[k].abs().max())
            assert float((t.double() - ref[k]).abs().max()) <= 1e-6 * scale, k
            assert float((t - plain[k]).abs().max()) <= 1e-6 * scale, k
    # a key prefix, the wrappers, a file, the official config.json beside it
    sdw = synth.make_istftnet_state_dict(cfg, weight_norm="g_v")
    want = IstftNet.from_state_dict(sdw, cfg).state_dict()

    def same(m):
        assert all(torch.equal(t, want[k]) for k, t in m.state_dict().items())

    pre = {"model.vocoder.generator." + k: v for k, v in sdw.items()}
    pre["model.stft.window"] = torch.ones(8)
    same(IstftNet.from_state_dict(pre, cfg))
    same(IstftNet.from_state_dict({"generator": sdw}, cfg))
    torch.save({"generator": sdw}, tmp_path / "g_0001")
    same(IstftNet.from_pretrained(tmp_path / "g_0001", cfg))
    official = {"resblock": "1", "num_mels": 20, "upsample_rates": [3, 2], "upsample_kernel_sizes": [7, 4],
                "upsample_initial_channel": 128, "resblock_kernel_sizes": [3, 11],
                "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]], "gen_istft_n_fft": 8, "gen_istft_hop_size": 2,
                "sampling_rate": 22050}
    (tmp_path / "config.json").write_text(json.dumps(official))
    beside = IstftNet.from_pretrained(tmp_path / "g_0001")
    same(beside)
    assert beside.config() == IstftNet(**cfg).config() and beside.hop_length == 12


def test_error_classes():
    cfg = DIMS["odd"]
    sd = synth.make_istftnet_state_dict(cfg)
    with pytest.raises(ValueError, match="does not fit the weights: gen_istft_n_fft 16"):
        IstftNet.from_state_dict(sd, dict(cfg, gen_istft_n_fft=16))
    with pytest.raises(ValueError, match="does not fit"):
        IstftNet.from_state_dict(sd, dict(cfg, upsample_rates=(3, 2, 2)))
    with pytest.raises(ValueError, match="does not fit"):
        IstftNet.from_state_dict(sd, dict(cfg, resblock_kernel_sizes=(3, 7)))
    with pytest.raises(ValueError, match="does not fit"):
        IstftNet.from_state_dict(sd, dict(cfg, resblock="2"))
    for drop in ("conv_post.weight", "conv_post.bias", "conv_pre.weight", "ups.1.weight", "resblocks.1.convs2.2.bias"):
        with pytest.raises(ValueError, match="missing keys"):
            IstftNet.from_state_dict({k: v for k, v in sd.items() if k != drop}, cfg)
    bad = dict(sd)
    bad["conv_post.bias"] = torch.zeros(9)
    with pytest.raises(ValueError, match="conv_post.bias: shape"):
        IstftNet.from_state_dict(bad, cfg)
    with pytest.raises(NotImplementedError, match="hop = n_fft / 4"):
        IstftNet.from_state_dict(sd, dict(cfg, gen_istft_hop_size=4))
    with pytest.raises(NotImplementedError, match="hop = n_fft / 4"):
        IstftNet(**dict(cfg, gen_istft_hop_size=1))
    with pytest.raises(NotImplementedError, match="gen_istft_n_fft 64"):
        IstftNet(**dict(cfg, gen_istft_n_fft=64, gen_istft_hop_size=16))
    with pytest.raises(NotImplementedError, match="gen_istft_n_fft 10"):
        IstftNet(**dict(cfg, gen_istft_n_fft=10))
    wide = dict(sd)
    wide["conv_post.weight"], wide["conv_post.bias"] = torch.zeros(66, 32, 7), torch.zeros(66)
    with pytest.raises(NotImplementedError, match="gen_istft_n_fft 64"):
        IstftNet.from_state_dict(wide, {k: v for k, v in cfg.items() if not k.startswith("gen_")})
    with pytest.raises(NotImplementedError, match="product of at least 2"):
        IstftNet(n_mels=20, upsample_initial_channel=64, upsample_rates=(1,), upsample_kernel_sizes=(3,))
    with pytest.raises(NotImplementedError, match="channel count 1024"):
        IstftNet(**dict(cfg, upsample_initial_channel=1024))
    with pytest.raises(NotImplementedError, match="fp32 and bf16"):
        IstftNet(**cfg).set_compute_dtype(torch.float16)
    m = IstftNet(**cfg)
    with pytest.raises(runtime.IspkError, match="GPU"):
        m(torch.zeros(1, 20, 4))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.istftnet_head(torch.zeros(8, 32), 8, torch.zeros(7, 18, 32), torch.zeros(18), runtime.istftnet_table(16), 16, 4,
                              torch.zeros(1, 32))


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    assert lib.ispk_istftnet_tile_frames() == runtime.ISTFTNET_TILE_FRAMES
    one = ctypes.c_void_p(16)      # never dereferenced: the checks fail first
    err = lambda: lib.ispk_last_error_string()
    head = lib.ispk_istftnet_head_f32
    args = lambda **kw: tuple({**dict(x=one, ldx=32, w=one, bias=one, table=one, table_floats=64, len=None, len_mul=1,
                                      audio=one, lda=36, alen=None, B=2, T=9, S=36, C=32, n_fft=16, hop=4, slope=0.01,
                                      phase_scale=1.0, stream=None), **kw}.values())
    assert head(*args(audio=None)) == E_NULL and b"null" in err()
    assert head(*args(w=None)) == E_NULL and head(*args(table=None)) == E_NULL and head(*args(x=None)) == E_NULL
    assert head(*args(C=8, ldx=8)) == E_UNSUP and b"channel count" in err()
    assert head(*args(C=544, ldx=544)) == E_UNSUP
    assert head(*args(n_fft=16, hop=8)) == E_UNSUP and b"geometry" in err()
    assert head(*args(n_fft=64, hop=16, table_floats=256, S=144, lda=144)) == E_UNSUP
    assert head(*args(n_fft=10, hop=2)) == E_UNSUP and head(*args(n_fft=4, hop=1)) == E_UNSUP
    assert head(*args(T=1, S=4, lda=4)) == E_SHAPE and b"T >= 2" in err()
    assert head(*args(T=0, S=0, lda=0)) == E_SHAPE
    assert head(*args(S=35)) == E_SHAPE and head(*args(lda=35)) == E_SHAPE
    assert head(*args(table_floats=63)) == E_SHAPE
    assert head(*args(B=70000)) == E_SHAPE and head(*args(len_mul=0)) == E_SHAPE
    assert head(*args(ldx=34)) == E_ALIGN and head(*args(x=ctypes.c_void_p(20))) == E_ALIGN
    assert head(*args(B=0, audio=None)) == 0


# ----------------------------------------------------------------------------------------- the GPU tests' inputs
def _mel(dims: str, case: str):
    B, T, lens, _ = CASES[case]
    mel = synth.make_vocoder_mel(B, DIMS[dims]["n_mels"], T, seed=len(case))
    return mel, lens if lens is not None else [T] * B


@pytest.mark.parametrize("dims", list(DIMS))
def test_gpu_inputs_are_informative(dims):
    """What make_istftnet_state_dict promises, per utterance of every case of tests/test_gpu_istftnet.py: exp is exercised well
    away from 1, sin past its linear part on both sides, the waveform neither near-silent nor huge."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cfg = DIMS[dims]
    m = ir.build(synth.make_istftnet_state_dict(cfg), cfg)
    H = cfg["gen_istft_n_fft"] // 2
    seen = 0
    for case in CASES:
        mel, lens = _mel(dims, case)
        for b, n in enumerate(lens):
            if n == 0:
                continue
            with torch.no_grad():
                audio, y = m(mel[b:b + 1, :, :n].double(), want_y=True)
            what = f"{dims}/{case} utterance {b}"
            assert audio.shape == (1, m.hop * n) and y.shape[2] == m.hop // m.istft_hop * n + 1, what
            peak, rms = float(audio.abs().max()), float(audio.pow(2).mean().sqrt())
            lo, hi = float(y[0, :H + 1].min()), float(y[0, :H + 1].max())
            a_lo, a_hi = float(y[0, H + 1:].min()), float(y[0, H + 1:].max())
            assert 0.1 < peak < 4.0 and rms > 0.04, f"{what}: peak {peak:.3f} rms {rms:.3f}"
            assert hi - lo > 4.0 and -7.0 < lo and hi < 4.0, f"{what}: log-magnitudes in [{lo:.2f}, {hi:.2f}]"
            assert a_lo < -math.pi / 2 and a_hi > math.pi / 2, f"{what}: sin's argument in [{a_lo:.2f}, {a_hi:.2f}]"
            seen += 1
    assert seen == 12


# ------------------------------------------------------------------------------------ the other generators' weights
def _digest(sd: dict) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(str(tuple(sd[k].shape)).encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def test_make_generator_default_output_is_unchanged():
    """Digests taken on the commit before `_make_generator` got `post_channels`."""
    assert _digest(synth.make_hifigan_state_dict()) == "a894f3f2981f34c102b42bf76662693ace6928de7dad6069c2d203eef0b7fdbe"
    assert _digest(synth.make_bigvgan_state_dict()) == "fbf52d419aa739239b8d95caec60dd7f2b10c008462b567186c397988469995a"
    assert _digest(synth.make_hifigan_state_dict(synth.HIFIGAN_DIMS["odd"], weight_norm="g_v")) == \
        "a685e59ab4619cf323f8b028e11fdb508294760d1d40a20cf5a28b29c30cff56"
