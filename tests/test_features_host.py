"""CPU: the host side of the feature extractor (isp_tts_amd.data): the restated slaney filterbank, the frame-count formulas,
from_config on the recipe's dataset section and its refusals, collate_audio, and argument errors without a GPU."""
import copy
import ctypes
import types
from collections.abc import Mapping

import numpy as np
import pytest
import torch

from isp_tts_amd import config, runtime, synth
from isp_tts_amd.data import AcousticFeatures, collate_audio, melscale_fbanks, pack_filterbank, pitch_frames, yin_lags

RECIPE_DATASET = config.ACOUSTIC_DATASET


def test_filterbank_matches_an_independent_slaney_implementation():
    audio_utils = pytest.importorskip("transformers.audio_utils")
    for sr, n_mels, f_min, f_max in ((22050, 80, 0.0, 8000.0), (16000, 64, 50.0, 7600.0), (24000, 100, 0.0, 12000.0)):
        ours = melscale_fbanks(513, f_min, f_max, n_mels, sr, "slaney", "slaney").double().numpy()
        ref = audio_utils.mel_filter_bank(513, n_mels, f_min, f_max, sr, norm="slaney", mel_scale="slaney")
        assert ours.shape == ref.shape == (513, n_mels)
        assert np.abs(ours - ref).max() <= 1e-7 * ref.max()          # (ours is rounded once to fp32)


def test_packed_filterbank_is_contiguous_and_fits():
    fb = melscale_fbanks(513, 0.0, 8000.0, 80, 22050)
    w, idx = pack_filterbank(fb)
    lo, off = idx[:80].tolist(), idx[80:].tolist()
    assert off[0] == 0 and off[-1] == w.numel() <= 2 * 513
    dense = torch.zeros_like(fb)
    for m in range(80):
        dense[lo[m]:lo[m] + off[m + 1] - off[m], m] = w[off[m]:off[m + 1]]
    assert torch.equal(dense, fb)


def test_frame_counts_match_unfold_on_the_reference_padding():
    """mel_len = (S + 768 - 1024) // 256 + 1 (torch.stft, center=False, on the 384-padded signal) and the YIN frame count
    (pitch.py:62-66 on the same padding) against unfold, for every S from 1 to 5000; the pitch count is mel_len - 1 exactly
    when S % 256 < 26 and S >= 282."""
    tau_min, tau_max = yin_lags(22050)
    assert (tau_min, tau_max) == (27, 525)
    for S in range(1, 5001):
        n = S + 768
        mel = torch.zeros(n).unfold(0, 1024, 256).shape[0] if n >= 1024 else 0
        assert runtime.feature_frames(S) == mel, S
        sig = n if n >= 2 * tau_max else 2 * tau_max
        yin = torch.zeros(sig).unfold(0, 2 * tau_max, 256).shape[0]
        assert pitch_frames(S, tau_max) == yin, S
        if S >= 256:
            assert (yin == mel - 1) == (S % 256 < 26 and S >= 282), S


def test_from_config_reads_the_recipe():
    f = AcousticFeatures.from_config(RECIPE_DATASET)
    assert (f.sample_rate, f.n_mels, f.tau_min, f.tau_max, f.threshold) == (22050, 80, 27, 525, 0.15)
    assert (f.pitch_mean, f.pitch_std, f.pitch, f.energy) == (166.6177, 62.5423, True, True)
    assert torch.equal(f.fb, melscale_fbanks(513, 0.0, 8000.0, 80, 22050))
    assert torch.equal(f.tables[4096:5120], torch.hann_window(1024))
    d = copy.deepcopy(RECIPE_DATASET)
    d["pitch"]["_disable_"] = True
    d["energy"] = None
    d.pop("stats")
    g = AcousticFeatures.from_config(d)
    assert not g.pitch and not g.energy and g.pitch_std == 1.0
    d = copy.deepcopy(RECIPE_DATASET)
    d["mel_scale"].update(n_mels=64, f_min=50.0, f_max=None)
    d["pitch"].update(f_max=600, threshold=0.1)
    g = AcousticFeatures.from_config(d)
    assert g.n_mels == 64 and g.tau_min == 36 and g.threshold == 0.1
    assert torch.equal(g.fb, melscale_fbanks(513, 50.0, 11025.0, 64, 22050))


class _Node(Mapping):
    """A read-only mapping that is not a dict, like OmegaConf's DictConfig (what the reference's recipe loader returns)."""

    def __init__(self, d):
        self._d = {k: _Node(v) if isinstance(v, dict) else v for k, v in d.items()}

    def __getitem__(self, k):
        return self._d[k]

    def __iter__(self):
        return iter(self._d)

    def __len__(self):
        return len(self._d)


def test_from_config_takes_any_mapping_and_stats_objects():
    """The recipe's dataset section as non-dict mappings at every level (stats and stats.pitch included) gives the same
    extractor as plain dicts; so do stats given as an AcousticDatasetStats-like object.  A stats file is refused."""
    want = AcousticFeatures.from_config(RECIPE_DATASET)
    node = _Node(RECIPE_DATASET)
    assert not isinstance(node, dict) and not isinstance(node["stats"], dict) and not isinstance(node["stats"]["pitch"], dict)
    for got in (AcousticFeatures.from_config(node),
                AcousticFeatures.from_config(dict(RECIPE_DATASET, stats=types.SimpleNamespace(
                    pitch=types.SimpleNamespace(mean=166.6177, std=62.5423))))):
        assert (got.pitch_mean, got.pitch_std, got.tau_min, got.tau_max, got.threshold) == \
            (want.pitch_mean, want.pitch_std, want.tau_min, want.tau_max, want.threshold) == (166.6177, 62.5423, 27, 525, 0.15)
        assert got.pitch and got.energy and torch.equal(got.tables, want.tables) and torch.equal(got.fb_index, want.fb_index)
    with pytest.raises(NotImplementedError):
        AcousticFeatures.from_config(dict(RECIPE_DATASET, stats="stats.json"))


@pytest.mark.parametrize("section, key, value", [
    ("spec", "n_fft", 2048), ("spec", "win_length", 800), ("spec", "hop_length", 200), ("spec", "center", True),
    ("spec", "power", 2.0), ("spec", "power", None), ("spec", "normalized", True), ("spec", "pad", 100),
    ("mel_scale", "mel_scale", "htk"), ("mel_scale", "norm", None), ("mel_scale", "n_mels", 200),
    ("pitch", "method", "penn"), ("pitch", "pad", 0), (None, "pitch_from_disk", True),
    ("audio", "sample_rate", 3000),
])
def test_from_config_refuses_what_is_not_built(section, key, value):
    d = copy.deepcopy(RECIPE_DATASET)
    (d[section] if section else d)[key] = value
    with pytest.raises(NotImplementedError):
        AcousticFeatures.from_config(d)


def test_collate_audio_pads_with_zeros():
    waves = [synth.make_clip("harmonic", 300, 0.5), synth.make_clip("noise", 1000, 0.5), synth.make_clip("chirp", 1, 0.5)]
    audio, lens = collate_audio(waves)
    assert audio.dtype == torch.float32 and audio.shape == (3, 1000) and lens.dtype == torch.int64
    assert lens.tolist() == [300, 1000, 1]
    for i, w in enumerate(waves):
        assert torch.equal(audio[i, :w.shape[0]], w) and not audio[i, w.shape[0]:].any()
    assert runtime.feature_frames(audio.shape[1]) == max(runtime.feature_frames(len(w)) for w in waves)
    with pytest.raises(ValueError):
        collate_audio([torch.zeros(2, 3)])


def test_clips_are_deterministic():
    for kind in synth.CLIP_KINDS:
        a, b = synth.make_clip(kind, 5000, 0.3), synth.make_clip(kind, 5000, 0.3)
        assert torch.equal(a, b) and a.dtype == torch.float32
        assert float(a.abs().max()) == pytest.approx(0.0 if kind == "silence" else 0.3, rel=1e-6)


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the checks fail first

    def rc(audio=one, ld=1024, lens=one, tables=one, tf=5847, fbi=one, n_mels=80, mel=one, B=2, S=1024, M=4, tmin=27, tmax=525,
           std=1.0):
        return lib.ispk_audio_features_f32(audio, ld, lens, tables, tf, fbi, n_mels, mel, one, one, one, B, S, M, tmin, tmax,
                                           22050.0, 0.15, 0.0, std, None)

    assert rc(audio=None) == -1 and rc(lens=None) == -1 and rc(tables=None) == -1 and rc(fbi=None) == -1
    assert b"null" in lib.ispk_last_error_string()
    assert rc(B=0) == -2 and rc(B=65536) == -2 and rc(ld=1000) == -2 and rc(S=-1) == -2
    assert rc(M=3) == -2 and b"frames" in lib.ispk_last_error_string()
    assert rc(n_mels=0) == -2 and rc(n_mels=129) == -2
    assert rc(tmax=683) == -2 and rc(tmin=0) == -2 and rc(tmin=524) == -2 and rc(tmax=500) == -2
    assert rc(std=0.0) == -2
    assert rc(tf=5119) == -2 and b"5120" in lib.ispk_last_error_string()
    with pytest.raises(runtime.IspkError):
        AcousticFeatures()(torch.zeros(2, 1024), torch.full((2,), 1024, dtype=torch.int64))
    with pytest.raises(ValueError):
        AcousticFeatures()(torch.zeros(2, 1024), torch.full((2,), 1024, dtype=torch.int32))
    with pytest.raises(ValueError):
        AcousticFeatures()(torch.zeros(2, 1024, dtype=torch.float64), torch.full((2,), 1024, dtype=torch.int64))
