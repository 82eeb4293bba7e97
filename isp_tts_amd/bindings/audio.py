"""Waveforms in and out: features, resampling, statistics and conditioning (csrc/features.hip, audio.hip, condition.hip), and
the Vocos, HiFi-GAN and BigVGAN vocoders (csrc/vocoder.hip, csrc/hifigan.hip, csrc/bigvgan.hip) with their denoiser
(csrc/denoise.hip) and the Griffin-Lim mel inversion (csrc/griffinlim.hip); the document join, speech marks, gain envelope and true-peak limiter
(csrc/join.hip, marks.hip, prosody.hip, limiter.hip); the equalizer (csrc/equalizer.hip)."""
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["FEATURE_HOP", "FEATURE_TABLE_HEAD", "feature_frames", "audio_features", "resampled_samples", "resample",
           "STATS_MAX_FRAMES", "feature_stats", "CONDITION_TABLE_DOUBLES", "CONDITION_MAX_SAMPLES", "CONDITION_RATES",
           "audio_measure_workspace_floats", "_mono_batch", "_out_like", "audio_measure", "audio_apply", "pcm16", "VOCODER_HOP",
           "VOCODER_TABLE_FLOATS", "_lengths_ptr", "vocoder_unfold", "dwconv7_ln", "istft_head", "HIFIGAN_TILE_ROWS",
           "HIFIGAN_MAX_CHANNELS", "HIFIGAN_MAX_KERNEL", "HIFIGAN_MAX_DILATION", "_hifigan_rows", "hifigan_conv", "_hifigan_bn",
           "hifigan_upsample", "hifigan_post", "SNAKE_AA_TILE_ROWS", "snake_aa", "DENOISE_TILE_SAMPLES", "DENOISE_N_FFT",
           "DENOISE_HOP", "DENOISE_TABLE_FLOATS", "denoise", "GRIFFINLIM_TILE_SAMPLES", "GRIFFINLIM_N_FFT", "GRIFFINLIM_HOP",
           "GRIFFINLIM_PAD", "GRIFFINLIM_STEP", "GRIFFINLIM_INIT", "mel_to_linear", "griffinlim_step", "griffinlim_fast_step",
           "griffinlim_error", "JOIN_TILE_SAMPLES", "JOIN_PLAN_BYTES", "JOIN_MAX", "JOIN_MAX_FADE", "join_plan", "join_audio",
           "MARKS_MAX_TOKENS", "MARKS_MAX_WORDS", "speech_marks", "GAIN_TILE_SAMPLES", "GAIN_MAX_RAMP", "gain_envelope",
           "LIMIT_TILE_SAMPLES", "LIMIT_MAX_LOOKAHEAD", "LIMIT_TAPS", "limit", "EQ_MAX_SECTIONS", "EQ_SEGMENT_SAMPLES",
           "EQ_CHUNK_SAMPLES", "EQ_TABLE_DOUBLES", "equalize_workspace_doubles", "equalize"]


FEATURE_HOP = 256          # STFT / YIN hop of ispk_audio_features_f32 (n_fft = win_length = 1024, pad 384 on each side)
FEATURE_TABLE_HEAD = 5120  # tables[0, 5120): W_2048^m as (re, im), then the Hann window; the filterbank weights follow


def feature_frames(samples: int) -> int:
    """Frames of an utterance of `samples` samples: (S + 768 - 1024) // 256 + 1, 0 below 256 samples (where torch.stft raises)."""
    return (samples - FEATURE_HOP) // FEATURE_HOP + 1 if samples >= FEATURE_HOP else 0


def audio_features(audio: Tensor, audio_len: Tensor, tables: Tensor, fb_index: Optional[Tensor], mel: Optional[Tensor],
                   mel_len: Optional[Tensor], pitch: Optional[Tensor], energy: Optional[Tensor], tau_min: int = 1,
                   tau_max: int = 512, sample_rate: float = 0.0, threshold: float = 0.0, pitch_mean: float = 0.0,
                   pitch_std: float = 1.0) -> None:
    """ispk_audio_features_f32, one launch, no host read: fills the given outputs (each may be None) of the fp32 waveforms
    audio [B, S] (unit stride on S, any row stride) with int64 lengths audio_len [B].  mel fp32 [B, n_mels, M], pitch / energy
    fp32 [B, M], mel_len int64 [B], all contiguous; tables fp32 and fb_index int32 as include/ispk.h lays them out
    (data.AcousticFeatures builds them).  The kernel reads no filterbank weight past tables.numel(), whatever fb_index
    (device data, not read here) says."""
    _rt._dev(audio, audio_len, tables, fb_index, mel, mel_len, pitch, energy)
    assert audio.dtype == torch.float32 and audio.ndim == 2 and audio.stride(1) == 1, "audio: fp32 [B, S], unit stride on S"
    assert audio_len.dtype == torch.int64 and audio_len.ndim == 1 and audio_len.is_contiguous()
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= FEATURE_TABLE_HEAD
    B, S = audio.shape
    if audio_len.shape[0] != B:
        raise ValueError(f"{audio_len.shape[0]} lengths for {B} waveforms")
    M, n_mels = None, 0
    for name, t, dt, nd in (("mel", mel, torch.float32, 3), ("pitch", pitch, torch.float32, 2),
                            ("energy", energy, torch.float32, 2), ("mel_len", mel_len, torch.int64, 1)):
        if t is None:
            continue
        if t.dtype != dt or t.ndim != nd or not t.is_contiguous() or t.shape[0] != B:
            raise ValueError(f"{name}: need a contiguous {dt} tensor of {nd} dims and {B} rows, got {t.dtype} {tuple(t.shape)}")
        if nd > 1:
            if M is not None and t.shape[-1] != M:
                raise ValueError(f"{name}: {t.shape[-1]} frames, another output has {M}")
            M = t.shape[-1]
    if mel is not None:
        n_mels = mel.shape[1]
        assert fb_index is not None and fb_index.dtype == torch.int32 and fb_index.numel() == 2 * n_mels + 1
    if B == 0:
        return
    _rt._launch("features_kernel", 0.0, 4.0 * audio.numel() + 4.0 * (n_mels + 2) * B * (M or 0), _rt.lib().ispk_audio_features_f32,
                audio.data_ptr(), audio.stride(0), audio_len.data_ptr(), tables.data_ptr(), tables.numel(), _rt._ptr(fb_index), n_mels, _rt._ptr(mel),
                _rt._ptr(mel_len), _rt._ptr(pitch), _rt._ptr(energy), B, S, M if M is not None else _rt.feature_frames(S), tau_min, tau_max,
                sample_rate, threshold, pitch_mean, pitch_std, _rt._stream())


def resampled_samples(samples: int, orig: int, dest: int) -> int:
    """ceil(dest * samples / orig): the output length of `samples` input samples at the reduced rates orig -> dest."""
    return (samples * dest + orig - 1) // orig


def resample(audio: Tensor, audio_len: Tensor, taps: Tensor, first: Tensor, orig: int, dest: int, width: int,
             out: Optional[Tensor] = None, out_len: Optional[Tensor] = None):
    """ispk_resample_f32, one launch, no host read: fp32 audio [B, S] or [B, C, S] (unit stride on S) with int64 lengths
    [B] -> (fp32 [B, ceil(dest S / orig)], int64 [B]); several channels are averaged.  `orig`, `dest` are the reduced rates,
    taps fp32 [dest, T] / first int32 [dest] the compact polyphase table (data.Resampler builds it)."""
    _rt._dev(audio, audio_len, taps, first, out, out_len)
    if audio.dtype != torch.float32 or audio.ndim not in (2, 3) or audio.stride(-1) != 1:
        raise ValueError(f"audio: fp32 [B, S] or [B, C, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} "
                         f"strides {tuple(audio.stride())}")
    B, S = audio.shape[0], audio.shape[-1]
    C = audio.shape[1] if audio.ndim == 3 else 1
    if audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous():
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    assert taps.dtype == torch.float32 and taps.ndim == 2 and taps.is_contiguous() and taps.shape[0] == dest
    assert first.dtype == torch.int32 and first.shape == (dest,) and first.is_contiguous()
    S_out = _rt.resampled_samples(S, orig, dest)
    if out is None:
        out = torch.empty((B, S_out), dtype=torch.float32, device=audio.device)
    if out_len is None:
        out_len = torch.empty((B,), dtype=torch.int64, device=audio.device)
    if out.dtype != torch.float32 or out.shape != (B, S_out) or out.stride(1) != 1:
        raise ValueError(f"out: fp32 [{B}, {S_out}] with unit stride on the samples, got {out.dtype} {tuple(out.shape)}")
    if out_len.dtype != torch.int64 or out_len.shape != (B,) or not out_len.is_contiguous():
        raise ValueError(f"out_len: contiguous int64 [{B}], got {out_len.dtype} {tuple(out_len.shape)}")
    if B == 0:
        return out, out_len
    _rt._launch("resample_kernel", 2.0 * taps.shape[1] * B * S_out, 4.0 * (B * C * S + B * S_out), _rt.lib().ispk_resample_f32,
                audio.data_ptr(), audio.stride(0), audio.stride(1) if audio.ndim == 3 else 0, audio_len.data_ptr(),
                taps.data_ptr(), taps.numel(), first.data_ptr(), out.data_ptr(), out.stride(0), out_len.data_ptr(), B, C, S, S_out,
                orig, dest, width, taps.shape[1], _rt._stream())
    return out, out_len


STATS_MAX_FRAMES = 4096    # ispk_feature_stats_f64 sorts an utterance in LDS


def feature_stats(pitch: Optional[Tensor], energy: Optional[Tensor], mel_len: Optional[Tensor], partial: Optional[Tensor],
                  state: Tensor, reset: bool = False) -> None:
    """ispk_feature_stats_f64, a launch pair, no host read: the per-utterance outlier-filtered (count, mean, M2, min, max) of
    pitch / energy fp32 [B, M] into partial float64 [B, 2, 5], folded in utterance order into state float64 [2, 5].  With
    pitch None (and reset) it only writes the empty state."""
    _rt._dev(pitch, energy, mel_len, partial, state)
    assert state.dtype == torch.float64 and state.shape == (2, 5) and state.is_contiguous()
    if pitch is None:
        _rt._launch("stats_fold_kernel", 0.0, 80.0, _rt.lib().ispk_feature_stats_f64, None, 0, None, 0, None, None, state.data_ptr(),
                    0, 0, int(reset), _rt._stream())
        return
    for name, t in (("pitch", pitch), ("energy", energy)):
        if t.dtype != torch.float32 or t.ndim != 2 or t.stride(1) != 1 or t.shape != pitch.shape:
            raise ValueError(f"{name}: fp32 {tuple(pitch.shape)} with unit stride on the frames, got {t.dtype} {tuple(t.shape)} "
                             f"strides {tuple(t.stride())}")
    B, M = pitch.shape
    if mel_len.dtype != torch.int64 or mel_len.shape != (B,) or not mel_len.is_contiguous():
        raise ValueError(f"mel_len: contiguous int64 [{B}], got {mel_len.dtype} {tuple(mel_len.shape)}")
    assert partial.dtype == torch.float64 and partial.shape == (B, 2, 5) and partial.is_contiguous()
    _rt._launch("feature_stats_kernel", 0.0, 8.0 * B * M, _rt.lib().ispk_feature_stats_f64, pitch.data_ptr(), pitch.stride(0),
                energy.data_ptr(), energy.stride(0), mel_len.data_ptr(), partial.data_ptr(), state.data_ptr(), B, M, int(reset),
                _rt._stream())


CONDITION_TABLE_DOUBLES = 152     # 7 coefficients, one unused, nine 4 x 4 powers of the state transition (include/ispk.h)
CONDITION_MAX_SAMPLES = 1 << 24
CONDITION_RATES = (8000, 768000)


def audio_measure_workspace_floats(B: int, S: int, sample_rate: int) -> int:
    """ispk_audio_measure_f64: per item the 256-sample square sums, the final states of every 32-sample chunk (4 doubles) and
    8,192-sample segment, 12 step partials and a peak per segment, and the step sums - in doubles, two floats each."""
    W, NH, NS = max(1, -(-S // 8192)), max(1, -(-S // 256)), S // (sample_rate // 10) + 1
    return 2 * B * (NH + W * (256 * 4 + 4 + 12 + 1) + NS)


def _mono_batch(audio: Tensor, audio_len: Optional[Tensor]) -> tuple[int, int]:
    if audio.dtype != torch.float32 or audio.ndim != 2 or audio.stride(1) != 1:
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    B, S = audio.shape
    if S > CONDITION_MAX_SAMPLES or B > 65535:
        raise ValueError(f"audio: at most 65535 utterances of {CONDITION_MAX_SAMPLES} samples, got {tuple(audio.shape)}")
    if audio_len is not None and (audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous()):
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    return B, S


def _out_like(name: str, t: Tensor, dtype, shape) -> None:
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or (t.ndim and t.stride(-1) != 1) or (t.ndim == 1 and not t.is_contiguous()):
        raise ValueError(f"{name}: {dtype} {tuple(shape)} with unit stride on the last axis, got {t.dtype} {tuple(t.shape)}")


def audio_measure(audio: Tensor, audio_len: Tensor, table: Tensor, sample_rate: int, trim_mode: int, trim_threshold: float,
                  pad_frames: int, gain_mode: int, target_lufs: float, peak_limit: float, bounds: Optional[Tensor] = None,
                  loudness: Optional[Tensor] = None, peak: Optional[Tensor] = None, gain: Optional[Tensor] = None):
    """ispk_audio_measure_f64, three launches, no host read: fp32 audio [B, S] (unit stride on S) with int64 lengths [B] ->
    (bounds int64 [B, 2], loudness float64 [B], peak fp32 [B], gain fp32 [B]).  `table` float64 [152] as include/ispk.h lays
    it out (data.AudioConditioner builds it)."""
    _rt._dev(audio, audio_len, table, bounds, loudness, peak, gain)
    B, S = _mono_batch(audio, audio_len)
    assert table.dtype == torch.float64 and table.shape == (CONDITION_TABLE_DOUBLES,) and table.is_contiguous()
    dev = audio.device
    bounds = torch.empty((B, 2), dtype=torch.int64, device=dev) if bounds is None else bounds
    loudness = torch.empty((B,), dtype=torch.float64, device=dev) if loudness is None else loudness
    peak = torch.empty((B,), dtype=torch.float32, device=dev) if peak is None else peak
    gain = torch.empty((B,), dtype=torch.float32, device=dev) if gain is None else gain
    _out_like("bounds", bounds, torch.int64, (B, 2))
    if not bounds.is_contiguous():
        raise ValueError("bounds: contiguous int64 [B, 2]")
    _out_like("loudness", loudness, torch.float64, (B,))
    _out_like("peak", peak, torch.float32, (B,))
    _out_like("gain", gain, torch.float32, (B,))
    if B == 0:
        return bounds, loudness, peak, gain
    ws = _rt.workspace(dev, _rt.audio_measure_workspace_floats(B, S, sample_rate))
    _rt._launch("audio_measure_kernels", 56.0 * B * S, 4.0 * 2 * B * S + 2.0 * 8 * B * S / 8, _rt.lib().ispk_audio_measure_f64, audio.data_ptr(),
                audio.stride(0), audio_len.data_ptr(), table.data_ptr(), table.numel(), bounds.data_ptr(), loudness.data_ptr(),
                peak.data_ptr(), gain.data_ptr(), ws.data_ptr(), ws.numel(), B, S, int(sample_rate), int(trim_mode),
                float(trim_threshold), int(pad_frames), int(gain_mode), float(target_lufs), float(peak_limit), _rt._stream())
    return bounds, loudness, peak, gain


def audio_apply(audio: Tensor, bounds: Tensor, gain: Optional[Tensor], out: Optional[Tensor] = None,
                out_len: Optional[Tensor] = None):
    """ispk_audio_apply_f32, one launch: out[b, i] = gain[b] * audio[b, start_b + i] below end_b - start_b, then zeros; the
    lengths go to out_len.  `out` fp32 [B, S_out] may not overlap `audio`."""
    _rt._dev(audio, bounds, gain, out, out_len)
    B, S = _mono_batch(audio, None)
    dev = audio.device
    out = torch.empty((B, S), dtype=torch.float32, device=dev) if out is None else out
    out_len = torch.empty((B,), dtype=torch.int64, device=dev) if out_len is None else out_len
    if out.ndim != 2:
        raise ValueError(f"out: fp32 [{B}, S_out], got {tuple(out.shape)}")
    _out_like("out", out, torch.float32, (B, out.shape[1]))
    _out_like("out_len", out_len, torch.int64, (B,))
    _out_like("bounds", bounds, torch.int64, (B, 2))
    if gain is not None:
        _out_like("gain", gain, torch.float32, (B,))
    if B == 0:
        return out, out_len
    _rt._launch("cond_apply_kernel", 1.0 * B * S, 4.0 * (B * S + out.numel()), _rt.lib().ispk_audio_apply_f32, audio.data_ptr(), audio.stride(0),
                bounds.data_ptr(), _rt._ptr(gain), out.data_ptr(), out.stride(0), out_len.data_ptr(), B, S, out.shape[1], _rt._stream())
    return out, out_len


def pcm16(audio: Tensor, audio_len: Tensor, dither: bool = False, seed: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """ispk_pcm16, one launch: fp32 [B, S] -> int16 [B, S], clamp(rint(32768 x + d)), zero past audio_len."""
    _rt._dev(audio, audio_len, out)
    B, S = _mono_batch(audio, audio_len)
    out = torch.empty((B, S), dtype=torch.int16, device=audio.device) if out is None else out
    _out_like("out", out, torch.int16, (B, S))
    if B == 0 or S == 0:
        return out
    _rt._launch("pcm16_kernel", 0.0, 6.0 * B * S, _rt.lib().ispk_pcm16, audio.data_ptr(), audio.stride(0), audio_len.data_ptr(),
                out.data_ptr(), out.stride(0), B, S, int(bool(dither)), int(seed) & 0xFFFFFFFFFFFFFFFF, _rt._stream())
    return out


# ------------------------------------------------------------------------------------------------- Vocos vocoder
VOCODER_HOP = 256             # ispk_istft_head_f32: n_fft 1024, hop 256, padding "same"
VOCODER_TABLE_FLOATS = 2 * 2048 + 1024


def _lengths_ptr(mel_len: Optional[Tensor], B: int) -> Optional[int]:
    if mel_len is None:
        return None
    if mel_len.dtype != torch.int64 or mel_len.shape != (B,) or not mel_len.is_contiguous():
        raise ValueError(f"mel_len: contiguous int64 [{B}], got {mel_len.dtype} {tuple(mel_len.shape)}")
    return mel_len.data_ptr()


def vocoder_unfold(mel: Tensor, mel_len: Optional[Tensor], rows: Tensor, row_mask: Optional[Tensor] = None) -> Tensor:
    """ispk_vocoder_unfold: mel fp32 / fp16 [B, C, T] (any strides) -> the embedding convolution's GEMM rows [B*T, K] (fp32 or
    bf16, K % 8 == 0, K >= 7 C; column j*C + c = tap j of channel c), zero past mel_len; row_mask bool [B*T] (t < mel_len)."""
    _rt._dev(mel, mel_len, rows, row_mask)
    assert mel.ndim == 3 and mel.dtype in (torch.float32, torch.float16)
    B, C, T = mel.shape
    assert rows.ndim == 2 and rows.shape[0] == B * T and rows.stride(1) == 1 and rows.dtype in (torch.float32, torch.bfloat16)
    assert row_mask is None or (row_mask.dtype == torch.bool and row_mask.numel() == B * T and row_mask.is_contiguous())
    K = rows.shape[1]
    ml = _lengths_ptr(mel_len, B)
    if B * T == 0:
        return rows
    _rt._launch(f"vocoder_unfold_kernel<{'f16' if mel.dtype == torch.float16 else 'f32'},"
                f"{'bf16' if rows.dtype == torch.bfloat16 else 'f32'}>", 0.0,
                float(mel.numel() * mel.element_size() + rows.numel() * rows.element_size() + B * T), _rt.lib().ispk_vocoder_unfold,
                mel.data_ptr(), int(mel.dtype == torch.float16), mel.stride(0), mel.stride(1), mel.stride(2), ml, rows.data_ptr(),
                int(rows.dtype == torch.bfloat16), rows.stride(0), _rt._ptr(row_mask), B, C, T, K, _rt._stream())
    return rows


def dwconv7_ln(x: Tensor, T: int, weight: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor, mel_len: Optional[Tensor],
               eps: float = 1e-6, out_dtype: torch.dtype = torch.float32, out: Optional[Tensor] = None) -> Tensor:
    """ispk_dwconv7_ln_f32: x fp32 [B*T, D] rows (unit column stride) -> LayerNorm(depthwise conv7(x)) fp32 / bf16 [B*T, D],
    each utterance's frames [0, mel_len) convolved alone, rows past mel_len zero.  weight fp32 [D, 7] contiguous."""
    _rt._dev(x, weight, bias, gamma, beta, mel_len, out)
    assert x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1
    R, D = x.shape
    B = R // T if T > 0 else 0
    assert B * T == R and weight.shape == (D, 7) and weight.is_contiguous()
    if out is None:
        out = torch.empty((R, D), dtype=out_dtype, device=x.device)
    assert out.shape == (R, D) and out.stride(1) == 1 and out.dtype in (torch.float32, torch.bfloat16)
    ml = _lengths_ptr(mel_len, B)
    if R == 0:
        return out
    _rt._launch(f"dwconv7_ln_kernel<{D // 64},{'bf16' if out.dtype == torch.bfloat16 else 'f32'}>", 18.0 * R * D,
                float(R * D * (4 + out.element_size())), _rt.lib().ispk_dwconv7_ln_f32, x.data_ptr(), x.stride(0), weight.data_ptr(),
                bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, ml, out.data_ptr(), int(out.dtype == torch.bfloat16),
                out.stride(0), B, T, D, _rt._stream())
    return out


def istft_head(h: Tensor, T: int, mel_len: Optional[Tensor], tables: Tensor, audio: Tensor,
               audio_len: Optional[Tensor] = None) -> Tensor:
    """ispk_istft_head_f32: the head Linear's fp32 rows h [B*T, >= 1026] (log-magnitudes in columns 0-512, phases in 513-1025)
    -> audio fp32 [B, S] (unit stride on S, S >= 256 T; zero from 256 mel_len on) and audio_len int64 [B] = 256 mel_len."""
    _rt._dev(h, mel_len, tables, audio, audio_len)
    assert h.dtype == torch.float32 and h.ndim == 2 and h.stride(1) == 1
    assert audio.dtype == torch.float32 and audio.ndim == 2 and audio.stride(1) == 1
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= VOCODER_TABLE_FLOATS
    B, S = audio.shape
    assert h.shape[0] == B * T
    assert audio_len is None or (audio_len.dtype == torch.int64 and audio_len.shape == (B,) and audio_len.is_contiguous())
    ml = _lengths_ptr(mel_len, B)
    if B == 0:
        return audio
    R = B * T
    _rt._launch("istft_head_kernel", R * 1.25 * (5.0 * 512 * 9 + 20.0 * 513), float(R * 1026 * 4 + B * S * 4),
                _rt.lib().ispk_istft_head_f32, h.data_ptr(), h.stride(0), ml, tables.data_ptr(), tables.numel(), audio.data_ptr(),
                audio.stride(0), _rt._ptr(audio_len), B, T, S, _rt._stream())
    return audio


# ------------------------------------------------------------------------------------------------- HiFi-GAN vocoder
HIFIGAN_TILE_ROWS = 128       # ispk_hifigan_tile_rows(): time positions per workgroup of the convolution kernels
HIFIGAN_MAX_CHANNELS = 512    # C_in, C_out: multiples of 32 up to this
HIFIGAN_MAX_KERNEL, HIFIGAN_MAX_DILATION = 11, 12


def _hifigan_rows(x: Tensor, name: str) -> None:
    assert x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1, f"{name}: fp32 rows [R, C] with unit column stride"


def hifigan_conv(x: Tensor, T: int, weight: Tensor, bias: Optional[Tensor], k: int, dilation: int = 1, slope: float = 1.0,
                 resid: Optional[Tensor] = None, out: Optional[Tensor] = None, accumulate: bool = False, scale: float = 1.0,
                 lengths: Optional[Tensor] = None, len_mul: int = 1) -> Tensor:
    """ispk_hifigan_conv_{f32,bf16} by weight.dtype: x fp32 [B*T, C_in] rows -> out fp32 [B*T, C_out] =
    [out +] scale * (bias + Conv1d(k, dilation, "same")(leaky_relu(x, slope)) [+ resid]); weight image [k, C_out, C_in].
    lengths int64 [B]: utterance b has lengths[b] * len_mul valid rows, the rest read and are written as zeros."""
    _rt._dev(x, weight, bias, resid, out, lengths)
    _hifigan_rows(x, "x")
    R, C_in = x.shape
    B = R // T if T > 0 else 0
    assert B * T == R and weight.ndim == 3 and weight.is_contiguous() and weight.shape[0] == k and weight.shape[2] == C_in
    assert weight.dtype in (torch.float32, torch.bfloat16)
    C_out = weight.shape[1]
    assert not accumulate or out is not None, "accumulate needs out="
    if out is None:
        out = torch.empty((R, C_out), dtype=torch.float32, device=x.device)
    _hifigan_rows(out, "out")
    assert out.shape == (R, C_out)
    if resid is not None:
        _hifigan_rows(resid, "resid")
        assert resid.shape == (R, C_out)
    ln = _lengths_ptr(lengths, B)
    if R == 0:
        return out
    bf = weight.dtype == torch.bfloat16
    _rt._launch(f"hifigan_conv_kernel<{'bf16' if bf else 'f32'},{_hifigan_bn(C_out)}>", 2.0 * R * C_out * C_in * k,
                float(R * 4 * (C_in + C_out * (1 + (resid is not None) + bool(accumulate))) + weight.numel() * weight.element_size()),
                _rt.lib().ispk_hifigan_conv_bf16 if bf else _rt.lib().ispk_hifigan_conv_f32, x.data_ptr(), x.stride(0), weight.data_ptr(),
                _rt._ptr(bias), _rt._ptr(resid), _rt._ld(resid), out.data_ptr(), out.stride(0), ln, len_mul, B,
                T, C_in, C_out, k, dilation, slope, scale, int(accumulate), _rt._stream())
    return out


def _hifigan_bn(C_out: int) -> int:
    return 128 if C_out % 128 == 0 else 64 if C_out % 64 == 0 else 32


def hifigan_upsample(x: Tensor, T: int, weight: Tensor, bias: Optional[Tensor], k: int, stride: int, slope: float = 0.1,
                     out: Optional[Tensor] = None, lengths: Optional[Tensor] = None, len_mul: int = 1) -> Tensor:
    """ispk_hifigan_upsample_{f32,bf16} by weight.dtype: x fp32 [B*T, C_in] rows -> out fp32 [B*T*stride, C_out] = bias +
    ConvTranspose1d(k, stride, padding (k - stride) / 2)(leaky_relu(x, slope)); weight image [k, C_out, C_in] (the module's
    [C_in, C_out, k] permuted).  lengths[b] * len_mul valid INPUT rows; output rows past stride times that are zeros."""
    _rt._dev(x, weight, bias, out, lengths)
    _hifigan_rows(x, "x")
    R, C_in = x.shape
    B = R // T if T > 0 else 0
    assert B * T == R and weight.ndim == 3 and weight.is_contiguous() and weight.shape[0] == k and weight.shape[2] == C_in
    assert weight.dtype in (torch.float32, torch.bfloat16)
    C_out = weight.shape[1]
    if out is None:
        out = torch.empty((R * stride, C_out), dtype=torch.float32, device=x.device)
    _hifigan_rows(out, "out")
    assert out.shape == (R * stride, C_out)
    ln = _lengths_ptr(lengths, B)
    if R == 0:
        return out
    bf = weight.dtype == torch.bfloat16
    _rt._launch(f"hifigan_conv_kernel<{'bf16' if bf else 'f32'},{_hifigan_bn(C_out)}>(T)", 2.0 * R * C_out * C_in * k,
                float(R * 4 * (C_in + C_out * stride) + weight.numel() * weight.element_size()),
                _rt.lib().ispk_hifigan_upsample_bf16 if bf else _rt.lib().ispk_hifigan_upsample_f32, x.data_ptr(), x.stride(0),
                weight.data_ptr(), _rt._ptr(bias), out.data_ptr(), out.stride(0), ln, len_mul, B, T, C_in, C_out, k, stride, slope,
                _rt._stream())
    return out


def hifigan_post(x: Tensor, T: int, weight: Tensor, bias: Tensor, audio: Tensor, audio_len: Optional[Tensor] = None,
                 lengths: Optional[Tensor] = None, len_mul: int = 1, slope: float = 0.01, final_clamp: bool = False) -> Tensor:
    """ispk_hifigan_post_f32: x fp32 [B*T, C] rows -> audio fp32 [B, S >= T] = tanh(bias + conv7(leaky_relu(x, slope))), zeros
    from lengths[b] * len_mul on; audio_len int64 [B] = lengths[b] * len_mul.  weight fp32 [7, C] contiguous, bias fp32 [1].
    final_clamp: ispk_hifigan_post_clamp_f32, clamp(., -1, 1) in place of tanh."""
    _rt._dev(x, weight, bias, audio, audio_len, lengths)
    _hifigan_rows(x, "x")
    assert audio.dtype == torch.float32 and audio.ndim == 2 and (audio.stride(1) == 1 or audio.shape[1] <= 1)
    B, S = audio.shape
    C = x.shape[1]
    assert x.shape[0] == B * T and weight.shape == (7, C) and weight.is_contiguous() and weight.dtype == torch.float32
    assert bias.dtype == torch.float32 and bias.numel() == 1
    assert audio_len is None or (audio_len.dtype == torch.int64 and audio_len.shape == (B,) and audio_len.is_contiguous())
    ln = _lengths_ptr(lengths, B)
    if B == 0:
        return audio
    _rt._launch("hifigan_post_kernel<clamp>" if final_clamp else "hifigan_post_kernel", 14.0 * B * T * C,
                float(B * T * C * 4 + B * S * 4), _rt.lib().ispk_hifigan_post_clamp_f32 if final_clamp else _rt.lib().ispk_hifigan_post_f32,
                _rt._ptr(x) if x.numel() else None, x.stride(0), weight.data_ptr(), bias.data_ptr(), ln, len_mul, audio.data_ptr(),
                max(audio.stride(0), S), _rt._ptr(audio_len), B, T, S, C, slope, _rt._stream())
    return audio


# --------------------------------------------------------------------------------------------------- BigVGAN vocoder
SNAKE_AA_TILE_ROWS = 512      # ispk_snake_aa_tile_rows(): rows of one utterance per workgroup of the activation kernel


def snake_aa(x: Tensor, T: int, al: Tensor, inv_b: Tensor, taps: Tensor, out: Optional[Tensor] = None,
             lengths: Optional[Tensor] = None, len_mul: int = 1) -> Tensor:
    """ispk_snake_aa_f32: x fp32 [B*T, C] rows -> out fp32 [B*T, C], the anti-aliased snake activation per utterance and
    channel: 2x upsampling with taps[:12] (replicate padding), u + inv_b sin(al u)^2, 2x low-pass downsampling with taps[12:].
    al, inv_b fp32 [C], taps fp32 [24], all contiguous.  lengths[b] * len_mul valid rows, the rest is never read and written
    as zeros.  Out of place only."""
    _rt._dev(x, al, inv_b, taps, out, lengths)
    _hifigan_rows(x, "x")
    R, C = x.shape
    B = R // T if T > 0 else 0
    assert B * T == R
    for name, t, n in (("al", al, C), ("inv_b", inv_b, C), ("taps", taps, 24)):
        assert t.dtype == torch.float32 and t.shape == (n,) and t.is_contiguous(), f"{name}: contiguous fp32 [{n}]"
    if out is None:
        out = torch.empty((R, C), dtype=torch.float32, device=x.device)
    _hifigan_rows(out, "out")
    assert out.shape == (R, C)
    ln = _lengths_ptr(lengths, B)
    if R == 0:
        return out
    _rt._launch("snake_aa_kernel", 56.0 * R * C, 8.0 * R * C, _rt.lib().ispk_snake_aa_f32, x.data_ptr(), x.stride(0),
                al.data_ptr(), inv_b.data_ptr(), taps.data_ptr(), out.data_ptr(), out.stride(0), ln, len_mul, B, T, C,
                _rt._stream())
    return out


# -------------------------------------------------------------------------------------------------- vocoder denoiser
DENOISE_TILE_SAMPLES = 4096   # ispk_denoise_tile_samples(): output samples of one utterance per workgroup
DENOISE_N_FFT, DENOISE_HOP = 1024, 256
DENOISE_TABLE_FLOATS = 2 * 2048 + 1024     # W_2048^m as (re, im), then the periodic Hann window, both made in float64


def denoise(audio: Tensor, audio_len: Optional[Tensor], tables: Tensor, bias: Tensor, strength,
            out: Optional[Tensor] = None) -> Tensor:
    """ispk_denoise_f32, one launch, no host read: fp32 audio [B, S] (unit stride on S, any row stride) with int64 lengths [B]
    (None: all S samples) -> out fp32 [B, S]: STFT (1024 / 256, periodic Hann, reflect-centred), every bin's magnitude less
    strength * bias[k] clamped at zero with the phase kept, ISTFT; zeros from audio_len on, utterances below 513 samples
    copied.  bias fp32 [513], tables fp32 [5120] (denoiser.Denoiser builds both); strength a float >= 0, or an fp32 [B] device
    tensor with one value per utterance.  Out of place only."""
    per_item = strength if isinstance(strength, Tensor) else None
    _rt._dev(audio, audio_len, tables, bias, per_item, out)
    if audio.dtype != torch.float32 or audio.ndim != 2 or audio.stride(1) != 1:
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    B, S = audio.shape
    if audio_len is not None and (audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous()):
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= DENOISE_TABLE_FLOATS
    assert bias.dtype == torch.float32 and bias.numel() == DENOISE_N_FFT // 2 + 1 and bias.is_contiguous()
    if per_item is not None:
        if per_item.dtype != torch.float32 or per_item.shape != (B,) or not per_item.is_contiguous():
            raise ValueError(f"strength: a float or a contiguous fp32 [{B}] tensor, got {per_item.dtype} {tuple(per_item.shape)}")
    elif not float(strength) >= 0.0:
        raise ValueError(f"strength: {strength} is negative or NaN")
    out = torch.empty((B, S), dtype=torch.float32, device=audio.device) if out is None else out
    _out_like("out", out, torch.float32, (B, S))
    if B == 0 or S == 0:
        return out
    # per hop: 19 / 16 of two 512-point transforms (9 radix passes of ~5 N flops) and the split / shrink / merge of 513 bins
    _rt._launch("denoise_kernel", B * S / 256.0 * (19.0 / 16.0) * (2 * 5.0 * 512 * 9 + 40.0 * 513), 8.0 * B * S,
                _rt.lib().ispk_denoise_f32, audio.data_ptr(), audio.stride(0), _rt._ptr(audio_len), tables.data_ptr(),
                bias.data_ptr(), _rt._ptr(per_item), 0.0 if per_item is not None else float(strength), out.data_ptr(),
                out.stride(0), B, S, _rt._stream())
    return out


# ----------------------------------------------------------------------------------------------- Griffin-Lim mel inversion
GRIFFINLIM_TILE_SAMPLES = 4096   # ispk_griffinlim_tile_samples(): output samples of one utterance per workgroup
GRIFFINLIM_N_FFT, GRIFFINLIM_HOP, GRIFFINLIM_PAD = 1024, 256, 384      # the feature extractor's framing
GRIFFINLIM_STEP, GRIFFINLIM_INIT = 0, 1                                # ISPK_GRIFFINLIM_STEP / _INIT


def _magnitude(mag: Tensor, B: int, T: int) -> None:
    bins = GRIFFINLIM_N_FFT // 2 + 1
    if (mag.dtype != torch.float32 or tuple(mag.shape) != (B, T, bins) or mag.stride(2) != 1 or mag.stride(1) != bins
            or (B > 1 and mag.stride(0) < T * bins)):
        raise ValueError(f"magnitude: fp32 [{B}, {T}, {bins}] with contiguous frame rows, got {mag.dtype} {tuple(mag.shape)} "
                         f"strides {tuple(mag.stride())}")


def mel_to_linear(mel: Tensor, mel_len: Optional[Tensor], pinv_t: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """ispk_mel_to_linear_f32, one launch, no host read: log-mel fp32 / fp16 [B, n_mels, T] (any strides) with int64 lengths [B]
    (None: all T frames) -> magnitude fp32 [B, T, 513] = max(P exp(mel), 0); frames at or past a length are neither read nor
    written.  pinv_t fp32 [n_mels, 513]: the transposed pseudo-inverse of the mel filterbank (griffinlim.GriffinLim builds it)."""
    _rt._dev(mel, mel_len, pinv_t, out)
    if mel.ndim != 3 or mel.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"mel: fp32 / fp16 [B, n_mels, T], got {mel.dtype} {tuple(mel.shape)}")
    B, C, T = mel.shape
    bins = GRIFFINLIM_N_FFT // 2 + 1
    assert pinv_t.dtype == torch.float32 and tuple(pinv_t.shape) == (C, bins) and pinv_t.is_contiguous()
    ml = _lengths_ptr(mel_len, B)
    out = torch.empty((B, T, bins), dtype=torch.float32, device=mel.device) if out is None else out
    _magnitude(out, B, T)
    if B == 0 or T == 0:
        return out
    _rt._launch(f"mel_to_linear_kernel<{'f16' if mel.dtype == torch.float16 else 'f32'}>", 2.0 * B * T * bins * C,
                float(mel.numel() * mel.element_size() + 4 * B * T * bins), _rt.lib().ispk_mel_to_linear_f32, mel.data_ptr(),
                int(mel.dtype == torch.float16), mel.stride(0), mel.stride(1), mel.stride(2), ml, pinv_t.data_ptr(),
                out.data_ptr(), out.stride(0), B, C, T, _rt._stream())
    return out


def griffinlim_step(audio: Optional[Tensor], mag: Tensor, mel_len: Optional[Tensor], tables: Tensor, out: Tensor,
                    audio_len: Optional[Tensor] = None, mode: int = GRIFFINLIM_STEP, seed: int = 0) -> Tensor:
    """ispk_griffinlim_step_f32, one launch, no host read.  mode GRIFFINLIM_STEP: one projection of fp32 audio [B, 256 T] (unit
    stride on the samples, any row stride) onto the magnitude mag fp32 [B, T, 513] - STFT in the extractor's framing (1024 /
    256, periodic Hann, 384 zeros on both sides), the magnitude replaced with the phase kept, ISTFT - into out fp32 [B, 256 T],
    out of place.  mode GRIFFINLIM_INIT: the ISTFT of mag with the phases hashed from (seed, frame, bin); audio is not read
    (None).  Zeros from 256 mel_len[b] on; audio_len int64 [B], if given, receives 256 mel_len.  tables fp32 [5120] as
    denoiser.denoise_tables() builds them."""
    _rt._dev(audio, mag, mel_len, tables, out, audio_len)
    if mode not in (GRIFFINLIM_STEP, GRIFFINLIM_INIT):
        raise ValueError(f"mode {mode}: GRIFFINLIM_STEP or GRIFFINLIM_INIT")
    if mag.ndim != 3:
        raise ValueError(f"magnitude: fp32 [B, T, 513], got {tuple(mag.shape)}")
    B, T = mag.shape[:2]
    _magnitude(mag, B, T)
    S = T * GRIFFINLIM_HOP
    if mode == GRIFFINLIM_STEP:
        if audio is None:
            raise ValueError("mode GRIFFINLIM_STEP needs the audio to project")
        _out_like("audio", audio, torch.float32, (B, S))
    else:
        audio = None
    _out_like("out", out, torch.float32, (B, S))
    ml = _lengths_ptr(mel_len, B)
    if audio_len is not None:
        _out_like("audio_len", audio_len, torch.int64, (B,))
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= DENOISE_TABLE_FLOATS
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed {seed}: an unsigned 64-bit value")
    if B == 0 or T == 0:
        return out
    # per hop: 20 / 16 of one (init) or two 512-point transforms (9 radix passes of ~5 N flops) and the projection of 513 bins
    ffts = 1 if mode == GRIFFINLIM_INIT else 2
    _rt._launch("griffinlim_kernel<init>" if mode == GRIFFINLIM_INIT else "griffinlim_kernel<step>",
                B * T * (20.0 / 16.0) * (ffts * 5.0 * 512 * 9 + 40.0 * 513), (4.0 * ffts + 4.0 * 513 / 256) * B * S,
                _rt.lib().ispk_griffinlim_step_f32, _rt._ptr(audio), 0 if audio is None else audio.stride(0), mag.data_ptr(),
                mag.stride(0), ml, tables.data_ptr(), out.data_ptr(), out.stride(0), _rt._ptr(audio_len), B, T, mode, int(seed),
                _rt._stream())
    return out


def griffinlim_fast_step(audio: Tensor, prev: Tensor, alpha: float, mag: Tensor, mel_len: Optional[Tensor], tables: Tensor,
                         out: Tensor, audio_len: Optional[Tensor] = None) -> Tensor:
    """ispk_griffinlim_fast_step_f32, one launch, no host read: griffinlim_step in mode GRIFFINLIM_STEP applied to audio - alpha
    prev, the fast (momentum) iteration with alpha = momentum / (1 + momentum) in [0, 1).  The STFT is linear, so this is the
    phase of STFT(audio) - alpha STFT(prev) without a spectrum in memory.  audio, prev and out are fp32 [B, 256 T] (unit stride
    on the samples, any row stride), out neither of the inputs; nothing at or past 256 mel_len[b] is read from audio or prev."""
    _rt._dev(audio, prev, mag, mel_len, tables, out, audio_len)
    if mag.ndim != 3:
        raise ValueError(f"magnitude: fp32 [B, T, 513], got {tuple(mag.shape)}")
    B, T = mag.shape[:2]
    _magnitude(mag, B, T)
    S = T * GRIFFINLIM_HOP
    _out_like("audio", audio, torch.float32, (B, S))
    _out_like("prev", prev, torch.float32, (B, S))
    _out_like("out", out, torch.float32, (B, S))
    ml = _lengths_ptr(mel_len, B)
    if audio_len is not None:
        _out_like("audio_len", audio_len, torch.int64, (B,))
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= DENOISE_TABLE_FLOATS
    if not 0.0 <= float(alpha) < 1.0:
        raise ValueError(f"alpha {alpha}: momentum / (1 + momentum), in [0, 1)")
    if B == 0 or T == 0:
        return out
    # griffinlim_step's count and bytes, with one more waveform read per sample
    _rt._launch("griffinlim_kernel<fast>", B * T * (20.0 / 16.0) * (2 * 5.0 * 512 * 9 + 40.0 * 513) + 2.0 * B * S,
                (12.0 + 4.0 * 513 / 256) * B * S, _rt.lib().ispk_griffinlim_fast_step_f32, audio.data_ptr(), audio.stride(0),
                prev.data_ptr(), prev.stride(0), float(alpha), mag.data_ptr(), mag.stride(0), ml, tables.data_ptr(),
                out.data_ptr(), out.stride(0), _rt._ptr(audio_len), B, T, _rt._stream())
    return out


def griffinlim_error(audio: Tensor, mag: Tensor, mel_len: Optional[Tensor], tables: Tensor, out: Optional[Tensor] = None,
                     work: Optional[Tensor] = None) -> Tensor:
    """ispk_griffinlim_error_f32, two launches, no host read, no atomics: the spectral convergence || |STFT(audio)| - mag ||_F /
    || mag ||_F per utterance, over its mel_len[b] frames, in griffinlim_step's framing -> out fp32 [B].  0 for an utterance
    without frames or with zero magnitude and zero audio, +inf for a zero magnitude under a non-zero spectrum.  work fp32
    [B, T, 2] (contiguous frame rows): the per-frame sums, scratch."""
    _rt._dev(audio, mag, mel_len, tables, out, work)
    if mag.ndim != 3:
        raise ValueError(f"magnitude: fp32 [B, T, 513], got {tuple(mag.shape)}")
    B, T = mag.shape[:2]
    _magnitude(mag, B, T)
    _out_like("audio", audio, torch.float32, (B, T * GRIFFINLIM_HOP))
    ml = _lengths_ptr(mel_len, B)
    out = torch.empty((B,), dtype=torch.float32, device=mag.device) if out is None else out
    _out_like("out", out, torch.float32, (B,))
    work = torch.empty((B, T, 2), dtype=torch.float32, device=mag.device) if work is None else work
    if (work.dtype != torch.float32 or tuple(work.shape) != (B, T, 2) or (T > 0 and tuple(work.stride()[1:]) != (2, 1))
            or (B > 1 and T > 0 and work.stride(0) < 2 * T)):
        raise ValueError(f"work: fp32 [{B}, {T}, 2] with contiguous frame rows, got {work.dtype} {tuple(work.shape)} strides "
                         f"{tuple(work.stride())}")
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.numel() >= DENOISE_TABLE_FLOATS
    if B == 0:
        return out
    if T == 0:
        return _rt.zero_(out)
    # per frame: one 512-point transform (9 radix passes of ~5 N flops) and ~20 flops for each of 513 bins; the pair is
    # labelled by its first kernel (the second reads 8 B per frame)
    _rt._launch("griffinlim_error_kernel", B * T * (5.0 * 512 * 9 + 20.0 * 513), (4.0 * 256 + 4.0 * 513 + 16.0) * B * T,
                _rt.lib().ispk_griffinlim_error_f32, audio.data_ptr(), audio.stride(0), mag.data_ptr(), mag.stride(0), ml,
                tables.data_ptr(), work.data_ptr(), work.stride(0), out.data_ptr(), B, T, _rt._stream())
    return out


# ------------------------------------------------------------------------------------------------------ document join
JOIN_TILE_SAMPLES = 4096      # ispk_join_tile_samples(): output samples of one document per workgroup
JOIN_PLAN_BYTES = 36864       # ispk_join_plan_bytes(): what ispk_join_plan hands to ispk_join_f32
JOIN_MAX = 1024               # items and documents per call
JOIN_MAX_FADE = 1 << 23


def join_plan(audio_len: Tensor, doc: Tensor, pos: Tensor, pause: Optional[Tensor], bounds: Optional[Tensor], plan: Tensor,
              item_offset: Tensor, item_len: Tensor, doc_len: Tensor, wanted_len: Tensor, S: int, S_out: int, fade: int = 0) -> None:
    """ispk_join_plan, one launch of one workgroup, no host read: orders the items of a batch by (doc, pos, b) and lays each
    document out (include/ispk.h has the arithmetic).  int64 [B]: audio_len, doc, pos, pause (None: zeros), item_offset,
    item_len; bounds int64 [B, 2] or None; int64 [D]: doc_len, wanted_len; plan: JOIN_PLAN_BYTES bytes of any dtype."""
    _rt._dev(audio_len, doc, pos, pause, bounds, plan, item_offset, item_len, doc_len, wanted_len)
    B, D = audio_len.shape[0], doc_len.shape[0]
    for name, t in (("audio_len", audio_len), ("doc", doc), ("pos", pos), ("pause", pause), ("item_offset", item_offset),
                    ("item_len", item_len)):
        if t is not None:
            _rt._out_like(name, t, torch.int64, (B,))
    if bounds is not None:
        _rt._out_like("bounds", bounds, torch.int64, (B, 2))
        if not bounds.is_contiguous():
            raise ValueError("bounds: contiguous int64 [B, 2]")
    _rt._out_like("doc_len", doc_len, torch.int64, (D,))
    _rt._out_like("wanted_len", wanted_len, torch.int64, (D,))
    if not plan.is_contiguous() or plan.numel() * plan.element_size() < JOIN_PLAN_BYTES:
        raise ValueError(f"plan: {JOIN_PLAN_BYTES} contiguous bytes, got {plan.numel() * plan.element_size()}")
    _rt._launch("join_plan_kernel", 0.0, 48.0 * B + JOIN_PLAN_BYTES, _rt.lib().ispk_join_plan, audio_len.data_ptr(), doc.data_ptr(),
                pos.data_ptr(), _rt._ptr(pause), _rt._ptr(bounds), plan.data_ptr(), plan.numel() * plan.element_size(),
                item_offset.data_ptr(), item_len.data_ptr(), doc_len.data_ptr(), wanted_len.data_ptr(), B, int(S), D, int(S_out),
                int(fade), _rt._stream())


def join_audio(audio: Tensor, gain: Optional[Tensor], plan: Tensor, doc_len: Tensor, out: Tensor) -> Tensor:
    """ispk_join_f32, one launch: gathers out fp32 [D, S_out] from audio fp32 [B, S] (unit stride on the samples, any row
    stride, both) by the plan and document lengths that `join_plan` wrote; gain fp32 [B] or None."""
    _rt._dev(audio, gain, plan, doc_len, out)
    B, S = audio.shape
    D, S_out = out.shape
    if gain is not None:
        _rt._out_like("gain", gain, torch.float32, (B,))
    _rt._launch("join_kernel", 3.0 * D * S_out, 4.0 * (B * S + D * S_out), _rt.lib().ispk_join_f32, audio.data_ptr(), audio.stride(0),
                _rt._ptr(gain), plan.data_ptr(), doc_len.data_ptr(), out.data_ptr(), out.stride(0), B, S, D, S_out, _rt._stream())
    return out


# ------------------------------------------------------------------------------------------------------ speech marks
MARKS_MAX_TOKENS = 4096       # tokens per item (L)
MARKS_MAX_WORDS = 1024        # words per item (W)


def speech_marks(duration: Tensor, text_len: Optional[Tensor], audio_len: Tensor, token_marks: Tensor,
                 word_marks: Optional[Tensor], hop: int, S: int, hard: bool = False, bounds: Optional[Tensor] = None,
                 item_offset: Optional[Tensor] = None, doc: Optional[Tensor] = None, doc_len: Optional[Tensor] = None,
                 doc_bounds: Optional[Tensor] = None, word_id: Optional[Tensor] = None) -> None:
    """ispk_speech_marks, one launch of one workgroup per item, no host read: the sample range of every token and word
    (include/ispk.h has the arithmetic).  duration fp32 [B, L] (unit stride on L, any row stride); int64 [B]: text_len (None:
    L tokens each), audio_len, item_offset, doc; bounds int64 [B, 2]; doc_len int64 [D]; doc_bounds int64 [D, 2]; word_id int64
    [B, L]; token_marks int64 [B, L, 2]; word_marks int64 [B, W, 2] or None (no words).  The join group (item_offset, doc,
    doc_len) is given whole or not at all."""
    _rt._dev(duration, text_len, audio_len, token_marks, word_marks, bounds, item_offset, doc, doc_len, doc_bounds, word_id)
    if duration.ndim != 2 or duration.dtype != torch.float32 or (duration.shape[1] > 1 and duration.stride(1) != 1):
        raise ValueError(f"duration: fp32 [B, L] with unit stride on L, got {duration.dtype} {tuple(duration.shape)} strides "
                         f"{tuple(duration.stride())}")
    B, L = duration.shape
    if B > 1 and duration.stride(0) < L:
        raise ValueError(f"duration: rows overlap (row stride {duration.stride(0)} < {L})")
    for name, t in (("text_len", text_len), ("audio_len", audio_len), ("item_offset", item_offset), ("doc", doc)):
        if t is not None:
            _rt._out_like(name, t, torch.int64, (B,))
    joined = [t is not None for t in (item_offset, doc, doc_len)]
    if any(joined) and not all(joined):
        raise ValueError("speech_marks: item_offset, doc and doc_len are given together or not at all")
    if doc_bounds is not None and not all(joined):
        raise ValueError("speech_marks: doc_bounds only together with item_offset, doc and doc_len")
    D = doc_len.shape[0] if doc_len is not None else 0
    W = word_marks.shape[1] if word_marks is not None and word_marks.ndim == 3 else 0
    for name, t, shape in (("bounds", bounds, (B, 2)), ("doc_len", doc_len, (D,)), ("doc_bounds", doc_bounds, (D, 2)),
                           ("word_id", word_id, (B, L)), ("token_marks", token_marks, (B, L, 2)), ("word_marks", word_marks, (B, W, 2))):
        if t is not None:
            _rt._out_like(name, t, torch.int64, shape)
            if not t.is_contiguous():
                raise ValueError(f"{name}: contiguous int64 {list(shape)}")
    if B == 0 or L == 0:
        return
    # read: the durations, word ids and the per-item / per-document scalars; written: both mark tensors
    nbytes = 4.0 * B * L + (8.0 * B * L if word_id is not None else 0.0) + 8.0 * (5 * B + 3 * D) + 16.0 * B * (L + W)
    _rt._launch("speech_marks_kernel", 2.0 * B * L, nbytes, _rt.lib().ispk_speech_marks, duration.data_ptr(),
                duration.stride(0) if B > 1 else max(duration.stride(0), L), _rt._ptr(text_len), audio_len.data_ptr(), _rt._ptr(bounds),
                _rt._ptr(item_offset), _rt._ptr(doc), _rt._ptr(doc_len), _rt._ptr(doc_bounds), _rt._ptr(word_id),
                token_marks.data_ptr(), _rt._ptr(word_marks) if W else None, int(hop), int(bool(hard)), B, L, int(S), D, W, _rt._stream())


# ------------------------------------------------------------------------------------------------------ gain envelope
GAIN_TILE_SAMPLES = 4096      # ispk_gain_envelope_tile_samples(): samples of one item per workgroup
GAIN_MAX_RAMP = 1 << 22


def gain_envelope(audio: Tensor, audio_len: Tensor, token_marks: Tensor, token_gain: Tensor, ramp: int, out: Tensor) -> Tensor:
    """ispk_gain_envelope_f32, one launch, no host read: out[b] = audio[b] * e, e the per-token gains token_gain fp32 [B, L]
    over the item-coordinate token_marks int64 [B, L, 2] with linear ramps of at most `ramp` samples on each side of a token
    boundary (include/ispk.h has the arithmetic).  audio and out fp32 [B, S] (unit stride on S, any row stride); out may be
    audio itself, otherwise the two do not overlap.  audio_len int64 [B]."""
    _rt._dev(audio, audio_len, token_marks, token_gain, out)
    if audio.dtype != torch.float32 or audio.ndim != 2 or (audio.shape[1] > 1 and audio.stride(1) != 1):
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    B, S = audio.shape
    if B > 65535 or S >= 2 ** 31:
        raise ValueError(f"audio: at most 65535 items of fewer than 2^31 samples, got {tuple(audio.shape)}")
    _out_like("audio_len", audio_len, torch.int64, (B,))
    if token_marks.ndim != 3:
        raise ValueError(f"token_marks: int64 [{B}, L, 2], got {tuple(token_marks.shape)}")
    L = token_marks.shape[1]
    _out_like("token_marks", token_marks, torch.int64, (B, L, 2))
    _out_like("token_gain", token_gain, torch.float32, (B, L))
    if not token_marks.is_contiguous() or not token_gain.is_contiguous():
        raise ValueError("token_marks and token_gain: contiguous")
    if not 1 <= L <= MARKS_MAX_TOKENS:
        raise ValueError(f"gain_envelope: 1 .. {MARKS_MAX_TOKENS} tokens, got {L}")
    if int(ramp) != ramp or not 0 <= ramp < GAIN_MAX_RAMP:
        raise ValueError(f"ramp is an integer in [0, 2^22), got {ramp!r}")
    _out_like("out", out, torch.float32, (B, S))
    if B > 1 and (audio.stride(0) < S or out.stride(0) < S):
        raise ValueError(f"audio / out: rows overlap (row strides {audio.stride(0)}, {out.stride(0)} < {S})")
    if B == 0 or S == 0:
        return out
    ld = lambda t: t.stride(0) if B > 1 else max(t.stride(0), S)      # noqa: E731
    _rt._launch("gain_envelope_kernel", 4.0 * B * S, 8.0 * B * S + 20.0 * B * L, _rt.lib().ispk_gain_envelope_f32, audio.data_ptr(),
                ld(audio), audio_len.data_ptr(), token_marks.data_ptr(), token_gain.data_ptr(), int(ramp), out.data_ptr(), ld(out), B,
                L, S, _rt._stream())
    return out


# ------------------------------------------------------------------------------------------------------ true-peak limiter
LIMIT_TILE_SAMPLES = 4096     # ispk_limit_tile_samples(): output samples of one item per workgroup
LIMIT_MAX_LOOKAHEAD = 256     # samples
LIMIT_TAPS = (4, 12)          # the interpolator: four phases of twelve taps


def limit(audio: Tensor, audio_len: Optional[Tensor], taps: Tensor, ceiling: float, lookahead: int, gain: Optional[Tensor] = None,
          bounds: Optional[Tensor] = None, out: Optional[Tensor] = None, out_len: Optional[Tensor] = None,
          true_peak: Optional[Tensor] = None, reduction: Optional[Tensor] = None, measure_only: bool = False):
    """ispk_limit_f32, one launch, no host read: the look-ahead limiter with a 4x oversampled (true-peak) detector on fp32 audio
    [B, S] (unit stride on S, any row stride) with int64 lengths [B] (None: S each), optional bounds int64 [B, 2] and gain fp32
    [B] (an AudioConditioner's), the interpolator taps fp32 [4, 12] (data.true_peak_taps), the linear ceiling and the look-ahead
    in samples (include/ispk.h has the arithmetic) -> (out fp32 [B, S], out_len int64 [B], true_peak fp32 [B], reduction fp32
    [B]).  `out` may not overlap `audio`.  measure_only: nothing but true_peak is computed or written -> (None, None, true_peak,
    None)."""
    _rt._dev(audio, audio_len, taps, gain, bounds, out, out_len, true_peak, reduction)
    B, S = _mono_batch(audio, audio_len)
    if taps.dtype != torch.float32 or tuple(taps.shape) != LIMIT_TAPS or not taps.is_contiguous():
        raise ValueError(f"taps: contiguous fp32 {list(LIMIT_TAPS)}, got {taps.dtype} {tuple(taps.shape)}")
    if int(lookahead) != lookahead or not 1 <= lookahead <= LIMIT_MAX_LOOKAHEAD:
        raise ValueError(f"lookahead is an integer in [1, {LIMIT_MAX_LOOKAHEAD}] samples, got {lookahead!r}")
    if not 0.0 < float(ceiling) < float("inf"):
        raise ValueError(f"ceiling is positive and finite (linear), got {ceiling!r}")
    if gain is not None:
        _out_like("gain", gain, torch.float32, (B,))
    if bounds is not None:
        _out_like("bounds", bounds, torch.int64, (B, 2))
        if not bounds.is_contiguous():
            raise ValueError("bounds: contiguous int64 [B, 2]")
    dev = audio.device
    true_peak = torch.empty((B,), dtype=torch.float32, device=dev) if true_peak is None else true_peak
    _out_like("true_peak", true_peak, torch.float32, (B,))
    if measure_only:
        if out is not None or out_len is not None or reduction is not None:
            raise ValueError("measure_only writes true_peak alone: out, out_len and reduction stay None")
    else:
        out = torch.empty((B, S), dtype=torch.float32, device=dev) if out is None else out
        out_len = torch.empty((B,), dtype=torch.int64, device=dev) if out_len is None else out_len
        reduction = torch.empty((B,), dtype=torch.float32, device=dev) if reduction is None else reduction
        if out.ndim != 2:
            raise ValueError(f"out: fp32 [{B}, {S}], got {tuple(out.shape)}")
        _out_like("out", out, torch.float32, (B, S))
        _out_like("out_len", out_len, torch.int64, (B,))
        _out_like("reduction", reduction, torch.float32, (B,))
        if B > 1 and out.stride(0) < S:
            raise ValueError(f"out: rows overlap (row stride {out.stride(0)} < {S})")
    if B > 1 and audio.stride(0) < S:
        raise ValueError(f"audio: rows overlap (row stride {audio.stride(0)} < {S})")
    if B == 0:
        return out, out_len, true_peak, reduction
    ld = lambda t: t.stride(0) if B > 1 else max(t.stride(0), S)      # noqa: E731
    # the envelope's 36 FMAs a sample; the smoothing sum only runs in tiles that hold a limited sample
    _rt._launch("limit_kernel", 72.0 * B * S, (4.0 if measure_only else 8.0) * B * S, _rt.lib().ispk_limit_f32, audio.data_ptr(),
                ld(audio), _rt._ptr(audio_len), _rt._ptr(bounds), _rt._ptr(gain), taps.data_ptr(), float(ceiling), int(lookahead),
                _rt._ptr(out), 0 if out is None else ld(out), _rt._ptr(out_len), true_peak.data_ptr(), _rt._ptr(reduction), B, S,
                _rt._stream())
    return out, out_len, true_peak, reduction


# ------------------------------------------------------------------------------------------------------ equalizer
EQ_MAX_SECTIONS = 8           # biquads in one cascade
EQ_SEGMENT_SAMPLES = 8192     # ispk_equalize_segment_samples(): samples of one item per workgroup, 256 chunks
EQ_CHUNK_SAMPLES = 32         # samples per lane; the table holds every section's A^(32 2^j), j = 0 .. 7


def EQ_TABLE_DOUBLES(sections: int) -> int:
    """Doubles of ispk_equalize_f32's table: per section 8 for the coefficients and eight 2 x 2 powers, then the joint
    2 N x 2 N A^8192 (include/ispk.h has the layout)."""
    return 40 * sections + 4 * sections * sections


def equalize_workspace_doubles(B: int, S: int, sections: int) -> int:
    """ispk_equalize_f32: the final joint state (2 N doubles) of every 8,192-sample segment of every item."""
    return B * max(1, -(-S // EQ_SEGMENT_SAMPLES)) * 2 * sections


def equalize(audio: Tensor, audio_len: Tensor, table: Tensor, sections: int, out: Optional[Tensor] = None,
             out_len: Optional[Tensor] = None, work: Optional[Tensor] = None):
    """ispk_equalize_f32, at most two launches, no host read: a cascade of `sections` (1 .. 8) float64 biquads over fp32 audio
    [B, S] (unit stride on S, any row stride) with int64 lengths [B] -> (out fp32 [B, S], zeros from each length on, out_len
    int64 [B] = the lengths).  `table` float64 [EQ_TABLE_DOUBLES(sections)] as include/ispk.h lays it out (data.Equalizer
    builds it); `work` float64, at least equalize_workspace_doubles(B, S, sections), scratch.  `out` may be `audio` itself (same
    base and row stride); any other overlap is refused."""
    _rt._dev(audio, audio_len, table, out, out_len, work)
    B, S = _mono_batch(audio, audio_len)
    if int(sections) != sections or not 1 <= sections <= EQ_MAX_SECTIONS:
        raise ValueError(f"sections is an integer in [1, {EQ_MAX_SECTIONS}], got {sections!r}")
    sections = int(sections)
    if table.dtype != torch.float64 or tuple(table.shape) != (EQ_TABLE_DOUBLES(sections),) or not table.is_contiguous():
        raise ValueError(f"table: contiguous float64 [{EQ_TABLE_DOUBLES(sections)}] for {sections} sections, got {table.dtype} "
                         f"{tuple(table.shape)}")
    dev = audio.device
    out = torch.empty((B, S), dtype=torch.float32, device=dev) if out is None else out
    out_len = torch.empty((B,), dtype=torch.int64, device=dev) if out_len is None else out_len
    if out.ndim != 2:
        raise ValueError(f"out: fp32 [{B}, {S}], got {tuple(out.shape)}")
    _out_like("out", out, torch.float32, (B, S))
    _out_like("out_len", out_len, torch.int64, (B,))
    if B > 1 and (audio.stride(0) < S or out.stride(0) < S):
        raise ValueError(f"audio / out: rows overlap (row strides {audio.stride(0)}, {out.stride(0)} < {S})")
    need = equalize_workspace_doubles(B, S, sections)
    work = torch.empty((max(need, 1),), dtype=torch.float64, device=dev) if work is None else work
    if work.dtype != torch.float64 or work.ndim != 1 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"work: contiguous float64 of at least {need} elements, got {work.dtype} {tuple(work.shape)}")
    if B == 0:
        return out, out_len
    ld = lambda t: t.stride(0) if B > 1 else max(t.stride(0), S)      # noqa: E731
    # per sample and section two runs of three FMAs, in both launches; read twice, written once
    _rt._launch("equalize_kernels", 24.0 * sections * B * S, 12.0 * B * S, _rt.lib().ispk_equalize_f32, audio.data_ptr(), ld(audio),
                audio_len.data_ptr(), table.data_ptr(), table.numel(), sections, out.data_ptr(), ld(out), out_len.data_ptr(),
                work.data_ptr(), work.numel(), B, S, _rt._stream())
    return out, out_len
