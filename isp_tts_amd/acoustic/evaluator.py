"""The acoustic model's evaluator (models/acoustic/evaluator.py of the reference): mel-cepstral distortion and the alignment
length / strength of the soft attention, with the reference's class names, call signatures and dict keys.

All three metrics come from ONE launch pair of ispk_acoustic_metrics_f32 (csrc/metrics.hip) and are 0-dim views of one device
buffer: no ATen compute op, no host read, so a training step that reports them can still be captured as a HIP graph
(train.GraphedTrainStep(..., evaluator=)).  The reference builds its DCT basis with torchaudio.functional.create_dct, which
is restated below from torchaudio's documented definition (torchaudio is not a dependency).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .. import runtime


def create_dct(n_mfcc: int, n_mels: int, norm: str | None = "ortho") -> Tensor:
    """torchaudio.functional.create_dct: the DCT-II basis as an fp32 [n_mels, n_mfcc] matrix (mels @ dct = the cepstrum),
    D[n, k] = cos(pi / n_mels (n + 1/2) k), times 2 (norm=None) or orthonormal (norm="ortho": column 0 by sqrt(1 / n_mels),
    the others by sqrt(2 / n_mels)).  Evaluated in float64 and rounded once."""
    if norm not in (None, "ortho"):
        raise ValueError('norm must be None or "ortho"')
    n = torch.arange(n_mels, dtype=torch.float64)
    k = torch.arange(n_mfcc, dtype=torch.float64).unsqueeze(1)
    dct = torch.cos(math.pi / n_mels * (n + 0.5) * k)               # [n_mfcc, n_mels]
    if norm is None:
        dct *= 2.0
    else:
        dct[0] *= 1.0 / math.sqrt(2.0)
        dct *= math.sqrt(2.0 / n_mels)
    return dct.t().contiguous().float()


def _field(obj, name: str):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


class MCD(torch.nn.Module):
    """Mel-cepstral distortion (evaluator.py:14-38): per frame the distance of the cepstra, coefficients 1 .. n_mfcc - 1,
    summed over ALL frames of an item (padding included), divided by its mel length, mean over the batch, in dB.
    A mel whose last size is n_mel_channels is read as [B, T, C], any other as [B, C, T] (the reference's `_mfcc` rule: a
    [B, C, C] mel is therefore read with its axes swapped)."""
    _logdb_const = 10.0 * np.sqrt(2.0) / np.log(10.0)

    def __init__(self, n_mel_channels: int = 80, n_mfcc: int = 13):
        super().__init__()
        self.n_mel_channels = n_mel_channels
        self.n_mfcc = n_mfcc  # number of mel-frequency cepstral coefficients
        self._dct_matrix = create_dct(self.n_mfcc, self.n_mel_channels, norm="ortho")
        self._dct_on: dict = {}

    def dct(self, device) -> Tensor:
        """The basis on `device` (copied once per device: the metric launches read it from there)."""
        device = torch.device(device)
        d = self._dct_on.get(device)
        if d is None:
            d = self._dct_on[device] = self._dct_matrix.to(device)
        return d

    def forward(self, mels_out: Tensor, mels_target: Tensor, mel_lengths: Tensor) -> Tensor:
        out = runtime.acoustic_metrics(mels_out, mels_target, mel_lengths, None, None, self.dct(mels_out.device))
        return out[0]


class AlignmentMetric(torch.nn.Module):
    """evaluator.py:41-64: -> (alignment_length, alignment_strength) of a soft alignment [B, T, L].  Length: per item the
    path length of the first-index argmax over frames 1 .. mel_len - 1, divided by the diagonal sqrt(text_len^2 + mel_len^2),
    mean over the batch.  Strength: the row maxima of all B * T frames over the summed mel lengths."""

    def __init__(self):
        super().__init__()

    def forward(self, alignments: Tensor, mel_lengths: Tensor, text_lengths: Tensor):
        out = runtime.acoustic_metrics(None, None, mel_lengths, text_lengths, alignments, None)
        return out[1], out[2]


class AcousticModelEvaluator:
    """evaluator.py:67-143.  `evaluator(inputs, outputs)` -> {"metrics/mcd_13", "metrics/alignment_length",
    "metrics/alignment_strength"}: 0-dim fp32 device tensors, views of one buffer written by one ispk_acoustic_metrics_f32
    call.  `inputs` is a dict (what `AcousticModel.prepare_inputs` returns) or any object with `mel`, `mel_len`, `text_len`;
    `outputs` the model's `AcousticModelOutput` (or a dict of its fields)."""

    def __init__(self, model=None):
        self.model = model

        self.mcd_evaluator = MCD()
        self.alignment_evaluator = AlignmentMetric()

    @torch.no_grad()
    def __call__(self, inputs, outputs) -> dict:
        mel_out = _field(outputs, "mel")
        attn_soft = _field(_field(outputs, "aligner_output"), "attn_soft")
        out = runtime.acoustic_metrics(mel_out, _field(inputs, "mel"), _field(inputs, "mel_len"), _field(inputs, "text_len"),
                                       attn_soft, self.mcd_evaluator.dct(mel_out.device))
        return {
            f"metrics/mcd_{self.mcd_evaluator.n_mfcc}": out[0],
            "metrics/alignment_length": out[1],
            "metrics/alignment_strength": out[2],
        }

    @torch.no_grad()
    def on_eval_epoch_end(self, inputs, outputs) -> dict:
        """evaluator.py:110-143: figures of item 0 of the collated batch (`filename`, `text_vector_len`, `mel`, `mel_len`):
        the soft and hard alignments [:mel_len, :text_len]^T, the target mel and the predicted mel clamped to the target's
        range -> {"images/eval/alignment": Figure, "images/eval/mel_spectrogram": Figure}.  Needs matplotlib."""
        idx = 0
        name = _field(inputs, "filename")[idx]
        text_len = int(_field(inputs, "text_vector_len")[idx])
        mel_len = int(_field(inputs, "mel_len")[idx])
        aligner = _field(outputs, "aligner_output")
        soft = _field(aligner, "attn_soft")[idx, :mel_len, :text_len].T
        hard = _field(aligner, "attn_hard")[idx, :mel_len, :text_len].T
        mel = _field(inputs, "mel")[idx, :, :mel_len]
        predicted = torch.clamp(_field(outputs, "mel")[idx, :, :mel_len], min=mel.min(), max=mel.max())
        return {
            "images/eval/alignment": _figure({"soft": soft, "hard": hard}, title=name, xlabel="Decoder timestep",
                                             ylabel="Encoder timestep"),
            "images/eval/mel_spectrogram": _figure({"target": mel, "predicted": predicted}, title=name, xlabel="Frames",
                                                   ylabel="Channels"),
        }


class SynthesisEvaluator:
    """Objective scores of free-running synthesis (`AcousticModel.infer`, which picks its own durations) against a recording:
    MCD after dynamic time warping, F0 RMSE in cents and voiced / unvoiced error along the same warping path, and the length
    ratio.  The reference has no counterpart (its evaluator is teacher-forced); the definitions are include/ispk.h's.

    `evaluator(mel_out, mel_out_len, mel_target, mel_target_len, pitch_out=None, pitch_target=None)` ->
    {"metrics/mcd_dtw_13", "metrics/f0_rmse_cents", "metrics/vuv_error", "metrics/length_ratio"}: 0-dim fp32 batch means,
    views of one device buffer written by one ispk_mcd_dtw_f32 call (the F0 keys only with both pitch tracks: fp32 [B, T] in
    Hz, 0 = unvoiced, what AcousticFeatures gives with pitch_mean=0, pitch_std=1).  `per_item=True`: the [B] vectors instead.
    The mels may differ in length and follow MCD's layout rule.  No ATen compute op and no host read: capturable."""

    def __init__(self, n_mel_channels: int = 80, n_mfcc: int = 13):
        self.mcd_evaluator = MCD(n_mel_channels, n_mfcc)

    @torch.no_grad()
    def __call__(self, mel_out: Tensor, mel_out_len: Tensor, mel_target: Tensor, mel_target_len: Tensor,
                 pitch_out: Optional[Tensor] = None, pitch_target: Optional[Tensor] = None, per_item: bool = False) -> dict:
        if (pitch_out is None) != (pitch_target is None):
            raise ValueError("give both pitch tracks or neither")
        items, means = runtime.mcd_dtw(mel_out, mel_out_len, mel_target, mel_target_len, self.mcd_evaluator.dct(mel_out.device),
                                       pitch_out, pitch_target)
        src = items if per_item else means
        out = {f"metrics/mcd_dtw_{self.mcd_evaluator.n_mfcc}": src[0]}
        if pitch_out is not None:
            out["metrics/f0_rmse_cents"] = src[1]
            out["metrics/vuv_error"] = src[2]
        out["metrics/length_ratio"] = src[3]
        return out

    @torch.no_grad()
    def score_infer(self, model, inputs, vocoder=None, features=None, per_item: bool = False, denoiser=None,
                    **infer_kwargs) -> dict:
        """`model.infer` on inputs["text"] / ["text_len"] (with ["speaker"] if present; `infer_kwargs` go to it: steps,
        flow_noise, max_dec_len ...), its mel and dec_lengths scored against inputs["mel"] / ["mel_len"].  With a Vocoder and
        an AcousticFeatures (pitch in Hz: pitch_mean=0, pitch_std=1) the mel is also vocoded, the waveform's pitch extracted and
        scored against inputs["pitch_hz"]; a `denoiser` (denoiser.Denoiser) is applied to the waveform between the two.
        Capturable with torch.cuda.graph when `max_dec_len` is given (infer's own rule)."""
        if (vocoder is None) != (features is None):
            raise ValueError("give both the vocoder and the feature extractor or neither")
        if denoiser is not None and vocoder is None:
            raise ValueError("a denoiser needs the vocoder whose waveform it cleans")
        if features is not None and (not features.pitch or features.pitch_mean != 0.0 or features.pitch_std != 1.0):
            raise ValueError("the feature extractor must deliver pitch in Hz (pitch=True, pitch_mean=0, pitch_std=1)")
        speaker = inputs.get("speaker") if isinstance(inputs, dict) else getattr(inputs, "speaker", None)
        if speaker is not None:
            infer_kwargs = {**infer_kwargs, "speaker": speaker}
        mel, adaptor = model.infer(_field(inputs, "text"), text_lengths=_field(inputs, "text_len"), **infer_kwargs)
        pitch_out = pitch_target = None
        if vocoder is not None:
            audio, audio_len = vocoder(mel, adaptor.dec_lengths)
            if denoiser is not None:
                audio, audio_len = denoiser(audio, audio_len)
            pitch_out, pitch_target = features(audio, audio_len)["pitch"], _field(inputs, "pitch_hz")
        return self(mel, adaptor.dec_lengths, _field(inputs, "mel"), _field(inputs, "mel_len"), pitch_out, pitch_target, per_item=per_item)


def _figure(panels: dict, title=None, xlabel=None, ylabel=None):
    """One row of image panels (origin at the bottom, as a spectrogram or an alignment is read), each with its colour bar."""
    from matplotlib.figure import Figure
    fig = Figure(figsize=(6 * len(panels), 3), constrained_layout=True)
    axes = fig.subplots(1, len(panels), squeeze=False)[0]
    for ax, (key, value) in zip(axes, panels.items()):
        im = ax.imshow(value.detach().float().cpu().numpy(), aspect="auto", origin="lower", interpolation="none")
        fig.colorbar(im, ax=ax)
        ax.set_title(key)
        if xlabel:
            ax.set_xlabel(xlabel)
        if ylabel:
            ax.set_ylabel(ylabel)
    if title is not None:
        fig.suptitle(str(title))
    return fig
