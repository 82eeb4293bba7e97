"""Generates tests/golden/features.npz: the REFERENCE data providers' features (tts/data/providers.py: SpectrogramProvider,
MelScaleProvider, EnergyProvider, the torch-yin PitchProvider; the pitch pad of tts/data/dataset.py:152; AcousticCollator of
tts/data/collator.py) on the clips of `synth.FEATURE_CASES`, with the recipe's settings (recipes/acoustic/core.yaml).

CPU only, run from the repository root where the reference exists (not on the GPU box):

    python3 tools/make_feature_goldens.py

The reference is imported read-only through `oracle/ref_shims`, like tools/make_metric_goldens.py.  Its torchaudio is a shim
there, so before `tts.data.providers` is imported this script puts restated `Spectrogram` and `MelScale` classes into the
shim's `torchaudio.transforms` module (in memory; the files under oracle/ are not touched): torchaudio's
functional.spectrogram (constant pad, torch.stft, magnitude) and MelScale (this project's melscale_fbanks, checked here
against transformers' independent slaney filterbank).  Everything else is the reference's own code on the real torch.  The
fixture holds the collated outputs and CRCs of the input clips only: the tests regenerate the clips from synth's streams.
"""
from __future__ import annotations

import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(1, "/root/reference")

import torchaudio.transforms as shim_transforms  # noqa: E402  (the shim)

from isp_tts_amd import synth  # noqa: E402
from isp_tts_amd.data import melscale_fbanks  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "features.npz")
RECIPE = dict(sample_rate=22050, n_mels=80, f_min=0.0, f_max=8000.0, pitch_f_max=800, threshold=0.15,
              pitch_mean=166.6177, pitch_std=62.5423)
torch.set_grad_enabled(False)


class Spectrogram(torch.nn.Module):
    """torchaudio.transforms.Spectrogram -> functional.spectrogram: constant pad of `pad` on both sides, torch.stft with
    window_fn(win_length) (torch.hann_window, periodic), then |X| ** power."""

    def __init__(self, n_fft=400, win_length=None, hop_length=None, pad=0, window_fn=torch.hann_window, power=2.0,
                 normalized=False, wkwargs=None, center=True, pad_mode="reflect", onesided=True, return_complex=None):
        super().__init__()
        self.n_fft, self.win_length = n_fft, win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.register_buffer("window", window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs))
        self.pad, self.power, self.normalized = pad, power, normalized
        self.center, self.pad_mode, self.onesided = center, pad_mode, onesided

    def forward(self, waveform):
        assert not self.normalized and self.power == 1.0
        if self.pad > 0:
            waveform = torch.nn.functional.pad(waveform, (self.pad, self.pad), "constant")
        shape = waveform.size()
        waveform = waveform.reshape(-1, shape[-1])
        spec = torch.stft(waveform, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                          window=self.window, center=self.center, pad_mode=self.pad_mode, normalized=False,
                          onesided=self.onesided, return_complex=True)
        spec = spec.reshape(shape[:-1] + spec.shape[-2:])
        return spec.abs()


class MelScale(torch.nn.Module):
    """torchaudio.transforms.MelScale: (spec^T @ fb)^T with fb = melscale_fbanks(n_stft, f_min, f_max, n_mels, sr, norm,
    mel_scale)."""

    def __init__(self, n_mels=128, sample_rate=16000, f_min=0.0, f_max=None, n_stft=201, norm=None, mel_scale="htk"):
        super().__init__()
        f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.register_buffer("fb", melscale_fbanks(n_stft, f_min, f_max, n_mels, sample_rate, norm, mel_scale))

    def forward(self, specgram):
        return torch.matmul(specgram.transpose(-1, -2), self.fb).transpose(-1, -2)


def crc(t) -> int:
    return zlib.crc32(np.ascontiguousarray(t.numpy()).tobytes())


def main():
    from transformers.audio_utils import mel_filter_bank
    fb = melscale_fbanks(513, 0.0, 8000.0, 80, 22050, "slaney", "slaney").double().numpy()
    tr = mel_filter_bank(513, 80, 0.0, 8000.0, 22050, norm="slaney", mel_scale="slaney")
    err = np.abs(fb - tr).max()
    print(f"melscale_fbanks vs transformers' mel_filter_bank: max |diff| = {err:.2e} (max weight {tr.max():.3e})")
    assert err < 1e-8

    shim_transforms.Spectrogram, shim_transforms.MelScale = Spectrogram, MelScale
    from tts.data import providers as dp       # (reference)
    from tts.data.collator import AcousticCollator
    from tts.data.dataset import AcousticSample

    r = RECIPE
    spec_p = dp.SpectrogramProvider(n_fft=1024, hop_length=256, win_length=1024, pad=None, power=1.0, normalized=False,
                                    center=False)
    mel_p = dp.MelScaleProvider(sample_rate=r["sample_rate"], n_fft=1024, n_mels=r["n_mels"], f_min=r["f_min"],
                                f_max=r["f_max"], norm="slaney", mel_scale="slaney")
    pitch_p = dp.PitchProvider(sample_rate=r["sample_rate"], hop_length=256, win_length=1024, f_min=40, f_max=r["pitch_f_max"],
                               method="torch-yin", threshold=r["threshold"], norm="standard")
    energy_p = dp.EnergyProvider()
    out = {}
    for case in synth.FEATURE_CASES:
        samples = []
        for i, audio in enumerate(synth.make_feature_case(case)):
            spec = spec_p(audio)                                      # dataset.py:140-156
            mel = mel_p(spec)
            pitch = pitch_p(audio, r["pitch_mean"], r["pitch_std"])
            pitch = torch.nn.functional.pad(pitch, (0, mel.shape[1] - pitch.size(0)))
            energy = energy_p(spec)
            samples.append(AcousticSample(filename=f"{case}{i}", text="", text_vector=torch.zeros(1, dtype=torch.long),
                                          text_vector_len=1, mel=mel, mel_len=mel.size(1), pitch=pitch, energy=energy))
        batch = AcousticCollator()(samples)
        for k in ("mel", "mel_len", "pitch", "energy"):
            out[f"{case}_{k}"] = batch[k].numpy()
        out[f"{case}_crc"] = np.array([crc(a) for a in synth.make_feature_case(case)], dtype=np.int64)
        print(f"{case:7s} mel {tuple(batch['mel'].shape)} mel_len {batch['mel_len'].tolist()}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
