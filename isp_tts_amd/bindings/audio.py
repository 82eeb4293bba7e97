"""Waveforms in and out: features, resampling, statistics and conditioning (csrc/features.hip, audio.hip, condition.hip);
the document join, speech marks, gain envelope and true-peak limiter (csrc/join.hip, marks.hip, prosody.hip, limiter.hip); the
equalizer (csrc/equalizer.hip); the segmenter (csrc/segment.hip); the screen (csrc/screen.hip); the declipper (csrc/declip.hip); the
noise reducer (csrc/noise.hip); the time stretch (csrc/stretch.hip); the pitch tracker (csrc/pyin.hip).  The vocoders' wrappers are in bindings/vocoders.py."""
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["FEATURE_HOP", "FEATURE_TABLE_HEAD", "feature_frames", "audio_features", "resampled_samples", "resample",
           "STATS_MAX_FRAMES", "feature_stats", "CONDITION_TABLE_DOUBLES", "CONDITION_MAX_SAMPLES", "CONDITION_RATES",
           "audio_measure_workspace_floats", "_mono_batch", "_out_like", "audio_measure", "audio_apply", "pcm16",
           "JOIN_TILE_SAMPLES", "JOIN_PLAN_BYTES", "JOIN_MAX", "JOIN_MAX_FADE", "join_plan", "join_audio", "MARKS_MAX_TOKENS",
           "MARKS_MAX_WORDS", "speech_marks", "GAIN_TILE_SAMPLES", "GAIN_MAX_RAMP", "gain_envelope", "LIMIT_TILE_SAMPLES",
           "LIMIT_MAX_LOOKAHEAD", "LIMIT_TAPS", "limit", "EQ_MAX_SECTIONS", "EQ_SEGMENT_SAMPLES", "EQ_CHUNK_SAMPLES",
           "EQ_TABLE_DOUBLES", "equalize_workspace_doubles", "equalize", "SEGMENT_MAX_SEGMENTS", "SEGMENT_MAX_ROWS", "SEGMENT_MAX_PAD",
           "SEGMENT_FLAGS", "segment_workspace_bytes", "segment_plan", "segment_gather", "SCREEN_TILE_SAMPLES", "SCREEN_TILE_FRAMES",
           "SCREEN_BINS", "SCREEN_FLAGS", "SCREEN_OUTPUTS", "screen_workspace_bytes", "screen", "DECLIP_SEGMENT_SAMPLES",
           "DECLIP_MAX_UNKNOWNS", "DECLIP_MAX_ORDER", "DECLIP_MAX_RUN", "DECLIP_MAX_ITERATIONS", "DECLIP_FLAGS", "DECLIP_OUTPUTS",
           "declip_workspace_bytes", "declip", "NOISE_TILE_SAMPLES", "NOISE_BINS",
           "NOISE_MIN_SAMPLES", "NOISE_MAX_GUARD", "NOISE_MAX_SMOOTH_FRAMES", "NOISE_MAX_SMOOTH_BINS", "NOISE_FLAGS", "NOISE_OUTPUTS",
           "noise_workspace_bytes", "noise_profile", "noise_reduce", "STRETCH_TILE_SAMPLES", "STRETCH_BINS", "STRETCH_MIN_SAMPLES",
           "STRETCH_RATES", "STRETCH_FLAGS", "stretch_workspace_bytes", "stretch", "PYIN_THRESHOLDS", "PYIN_MAX_BINS", "PYIN_MAX_TROUGHS",
           "PYIN_TABLE_DOUBLES", "PYIN_MAX_PERIOD", "PYIN_MAX_WIDTH", "PYIN_FRAMES_PER_BLOCK", "pyin_workspace_bytes", "pyin_observe",
           "pyin_decode"]


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


# ------------------------------------------------------------------------------------------------------ segmenter
SEGMENT_MAX_SEGMENTS = 4096   # K: stored segments per item
SEGMENT_MAX_ROWS = 65535      # R: rows of one gather
SEGMENT_MAX_PAD = 65536       # frames
SEGMENT_FLAGS = {"over": 1, "short": 2, "cut": 4}      # longer than max_samples; shorter than min_samples; cut at S_out (rows only)
_SEGMENT_PLAN = (("segments", torch.int64, 2), ("flags", torch.int32, 0), ("frames", torch.int32, 0), ("speech_frames", torch.int32, 0),
                 ("speech_power", torch.float64, 0), ("noise_power", torch.float64, 0))
_SEGMENT_ROWS = (("audio_len", torch.int64, 0), ("item", torch.int32, 0), ("index", torch.int32, 0), ("bounds", torch.int64, 2),
                 ("row_flags", torch.int32, 0))


def segment_workspace_bytes(B: int, S: int) -> int:
    """ispk_segment_workspace_bytes: per item the 256-sample square sums and the frame powers (float64 each) and (e, s) int64 of
    up to NH / 5 + 1 candidates."""
    NH = max(1, -(-S // 256))
    return 8 * B * (2 * NH + 2 * (NH // 5 + 1))


def _segment_audio(audio: Tensor) -> tuple[int, int]:
    if audio.dtype != torch.float32 or audio.ndim != 2 or (audio.shape[1] > 1 and audio.stride(1) != 1):
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    B, S = audio.shape
    if B > 65535 or S >= 2 ** 31:
        raise ValueError(f"audio: at most 65535 items of fewer than 2^31 samples, got {tuple(audio.shape)}")
    if B > 1 and audio.stride(0) < S:
        raise ValueError(f"audio: rows overlap (row stride {audio.stride(0)} < {S})")
    return B, S


def _segment_tensors(spec, lead: tuple, given: Optional[dict], device) -> dict:
    """The tensors of `spec` = (name, dtype, trailing 2 or 0) with the leading shape `lead`: taken from `given`, checked, or made."""
    out = {}
    for name, dt, two in spec:
        shape = lead + ((2,) if two else ())
        t = None if given is None else given.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=device)
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: contiguous {dt} {list(shape)}, got {t.dtype} {tuple(t.shape)}")
        out[name] = t
    return out


def segment_plan(audio: Tensor, audio_len: Tensor, factor: float, ref_mode: int, ref: float, pad: int, min_silence_frames: int,
                 target_samples: int, max_samples: int, min_samples: int, max_segments: int, out: Optional[dict] = None) -> dict:
    """ispk_segment_plan, two launches, no host read: where to cut fp32 audio [B, S] (unit stride on S, any row stride) with int64
    lengths [B] (include/ispk.h has the arithmetic) -> a dict of segments int64 [B, K, 2]; flags, frames, speech_frames int32
    [B, K]; speech_power, noise_power float64 [B, K]; count, wanted int32 [B]; work (uint8 scratch of segment_workspace_bytes).
    `out` may hold any of them; the rest is allocated."""
    B, S = _segment_audio(audio)
    K = int(max_segments)
    if not 1 <= K <= SEGMENT_MAX_SEGMENTS:
        raise ValueError(f"max_segments is an integer in [1, {SEGMENT_MAX_SEGMENTS}], got {max_segments!r}")
    dev = audio.device
    r = _segment_tensors(_SEGMENT_PLAN, (B, K), out, dev)
    r.update(_segment_tensors((("count", torch.int32, 0), ("wanted", torch.int32, 0)), (B,), out, dev))
    need = segment_workspace_bytes(B, S)
    work = None if out is None else out.get("work")
    work = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev) if work is None else work
    if work.dtype != torch.uint8 or work.ndim != 1 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"work: contiguous uint8 of at least {need} bytes, got {work.dtype} {tuple(work.shape)}")
    r["work"] = work
    _rt._dev(audio, audio_len, *r.values())
    if audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous():
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    # read once for the hop sums; the per-item pass moves 16 B a frame, a few times over
    _rt._launch("segment_plan_kernels", 2.0 * B * S, 4.0 * B * S + 64.0 * B * (S // 256), _rt.lib().ispk_segment_plan, audio.data_ptr(),
                audio.stride(0) if B > 1 else max(audio.stride(0), S), audio_len.data_ptr(), float(factor), int(ref_mode), float(ref),
                int(pad), int(min_silence_frames), int(target_samples), int(max_samples), int(min_samples), r["segments"].data_ptr(),
                r["flags"].data_ptr(), r["count"].data_ptr(), r["wanted"].data_ptr(), r["frames"].data_ptr(),
                r["speech_frames"].data_ptr(), r["speech_power"].data_ptr(), r["noise_power"].data_ptr(), work.data_ptr(),
                work.numel(), B, S, K, _rt._stream())
    return r


def segment_gather(audio: Tensor, segments: Tensor, flags: Tensor, count: Tensor, drop: int, rows: int, samples: int,
                   out: Optional[dict] = None) -> dict:
    """ispk_segment_gather_f32, two launches, no host read: the stored segments of a plan without a flag of the mask `drop`, in
    (item, index) order, into the rows of audio fp32 [R, S_out] -> a dict of audio; audio_len int64 [R]; item, index, row_flags
    int32 [R]; bounds int64 [R, 2]; rows, rows_wanted int32 [1].  `out` may hold any of them; out["audio"] may have any row
    stride and may not overlap `audio`."""
    B, S = _segment_audio(audio)
    R, S_out = int(rows), int(samples)
    if not 0 <= R <= SEGMENT_MAX_ROWS or not 0 <= S_out < 2 ** 31:
        raise ValueError(f"rows in [0, {SEGMENT_MAX_ROWS}] and samples in [0, 2^31), got {rows!r}, {samples!r}")
    if segments.ndim != 3:
        raise ValueError(f"segments: int64 [{B}, K, 2], got {tuple(segments.shape)}")
    K = segments.shape[1]
    _segment_tensors((("segments", torch.int64, 2), ("flags", torch.int32, 0)), (B, K), dict(segments=segments, flags=flags), None)
    _segment_tensors((("count", torch.int32, 0),), (B,), dict(count=count), None)
    dev = audio.device
    r = _segment_tensors(_SEGMENT_ROWS, (R,), out, dev)
    r.update(_segment_tensors((("rows", torch.int32, 0), ("rows_wanted", torch.int32, 0)), (1,), out, dev))
    o = None if out is None else out.get("audio")
    o = torch.empty((R, S_out), dtype=torch.float32, device=dev) if o is None else o
    if o.dtype != torch.float32 or tuple(o.shape) != (R, S_out) or (S_out > 1 and o.stride(1) != 1) or (R > 1 and o.stride(0) < S_out):
        raise ValueError(f"out audio: fp32 [{R}, {S_out}] with unit stride on the samples, got {o.dtype} {tuple(o.shape)} strides "
                         f"{tuple(o.stride())}")
    r["audio"] = o
    _rt._dev(audio, segments, flags, count, *r.values())
    _rt._launch("segment_gather_kernels", 0.0, 8.0 * R * S_out, _rt.lib().ispk_segment_gather_f32, audio.data_ptr(),
                audio.stride(0) if B > 1 else max(audio.stride(0), S), segments.data_ptr(), flags.data_ptr(), count.data_ptr(), int(drop),
                o.data_ptr(), o.stride(0) if R > 1 else max(o.stride(0), S_out), r["audio_len"].data_ptr(), r["item"].data_ptr(),
                r["index"].data_ptr(), r["bounds"].data_ptr(), r["row_flags"].data_ptr(), r["rows"].data_ptr(),
                r["rows_wanted"].data_ptr(), B, S, K, R, S_out, _rt._stream())
    return r


# ------------------------------------------------------------------------------------------------------ screen
SCREEN_TILE_SAMPLES = 4096    # ispk_screen_tile_samples(): samples of one item per workgroup
SCREEN_TILE_FRAMES = 16       # the frames (1024 / 256, no padding) that start in a tile
SCREEN_BINS = 513
SCREEN_FLAGS = {"clipped": 1, "narrow": 2, "dc": 4, "dropout": 8, "nonfinite": 16, "quiet": 32, "short": 64}
# name, dtype, trailing dimension (0: none), in the order of ispk_screen_f64's output pointers
SCREEN_OUTPUTS = (("nonfinite", torch.int32, 0), ("peak", torch.float32, 0), ("dc", torch.float64, 0), ("power", torch.float64, 0),
                  ("clip_runs", torch.int32, 0), ("clip_samples", torch.int64, 0), ("clip_longest", torch.int64, 0),
                  ("clip_first", torch.int64, 0), ("dropout_runs", torch.int32, 0), ("dropout_samples", torch.int64, 0),
                  ("dropout_longest", torch.int64, 0), ("ltas", torch.float64, SCREEN_BINS), ("band_bin", torch.int32, 0),
                  ("flags", torch.int32, 0))


def screen_workspace_bytes(B: int, S: int) -> int:
    """ispk_screen_workspace_bytes: per item and tile of 4,096 samples a float64 spectrum partial [513], the tile's statistics and
    two run summaries (11 more 8-byte words), and one word per item."""
    return 8 * B * ((SCREEN_BINS + 11) * max(1, -(-S // SCREEN_TILE_SAMPLES)) + 1)


def screen(audio: Tensor, audio_len: Tensor, tables: Tensor, rail_mode: int, rail: float, rail_ratio: float, min_run: int,
           min_dropout: int, band_factor: float, min_band_bin: int, max_dc: float, min_peak: float, out: Optional[dict] = None,
           parts: int = 3) -> dict:
    """ispk_screen_f64, four launches, no host read: the measurements and flags (include/ispk.h has the definitions) of fp32 audio
    [B, S] (unit stride on S, any row stride) with int64 lengths [B] -> a dict of the SCREEN_OUTPUTS, [B] each and ltas
    float64 [B, 513], and work (uint8 scratch of screen_workspace_bytes).  tables: fp32, W_2048 and the window in front (data.
    AcousticFeatures' or the denoiser's).  min_band_bin -1: no bandwidth floor.  `out` may hold any of them; the rest is allocated."""
    B, S = _segment_audio(audio)
    if S > CONDITION_MAX_SAMPLES:
        raise ValueError(f"audio: at most {CONDITION_MAX_SAMPLES} samples an item, got {tuple(audio.shape)}")
    dev = audio.device
    r = {}
    for name, dt, last in SCREEN_OUTPUTS:
        r.update(_segment_tensors(((name, dt, 0),), (B, last) if last else (B,), out, dev))
    need = screen_workspace_bytes(B, S)
    work = None if out is None else out.get("work")
    work = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev) if work is None else work
    if work.dtype != torch.uint8 or work.ndim != 1 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"work: contiguous uint8 of at least {need} bytes, got {work.dtype} {tuple(work.shape)}")
    if audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous():
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() < FEATURE_TABLE_HEAD:
        raise ValueError(f"tables: contiguous fp32 of at least {FEATURE_TABLE_HEAD} values, got {tables.dtype} {tuple(tables.shape)}")
    _rt._dev(audio, audio_len, tables, work, *r.values())
    # per frame five radix passes of 512 complex points and the split; the audio is read twice (the halo apart)
    frames = B * max(0, (S - 1024) // FEATURE_HOP + 1)
    _rt._launch("screen_kernels", frames * (5.0 * 512 * 9 + 513 * 12), 8.0 * B * S + 16.0 * frames / SCREEN_TILE_FRAMES * SCREEN_BINS,
                _rt.lib().ispk_screen_f64, audio.data_ptr(), audio.stride(0) if B > 1 else max(audio.stride(0), S), audio_len.data_ptr(),
                tables.data_ptr(), int(parts), int(rail_mode), float(rail), float(rail_ratio), int(min_run), int(min_dropout),
                float(band_factor), int(min_band_bin), float(max_dc), float(min_peak), *(r[name].data_ptr() for name, _, _ in SCREEN_OUTPUTS),
                work.data_ptr(), work.numel(), B, S, _rt._stream())
    r["work"] = work
    return r


# ------------------------------------------------------------------------------------------------------ declipper
DECLIP_SEGMENT_SAMPLES = 512  # samples of one item per workgroup of the solve; its window reaches 256 further on either side
DECLIP_MAX_UNKNOWNS = 256     # ispk_declip_max_unknowns(): a window with more unknown samples is left as it is (dense)
DECLIP_MAX_ORDER, DECLIP_MAX_RUN, DECLIP_MAX_ITERATIONS = 32, 64, 8
DECLIP_FLAGS = {"restored": 1, "dense": 2, "skipped": 4}
# name, dtype, trailing dimension (0: none), in the order of ispk_declip_f64's output pointers behind out
DECLIP_OUTPUTS = (("audio_len", torch.int64, 0), ("thr", torch.float32, 0), ("peak", torch.float32, 0), ("clip_samples", torch.int64, 0),
                  ("restored", torch.int64, 0), ("windows", torch.int32, 0), ("dense", torch.int32, 0), ("flags", torch.int32, 0))


def declip_workspace_bytes(B: int, S: int) -> int:
    """ispk_declip_workspace_bytes: per item 16 B per segment of 512 samples and 4 B per tile of 4,096, rounded up to 8 B."""
    return 8 * B * (2 * max(1, -(-S // DECLIP_SEGMENT_SAMPLES)) + (max(1, -(-S // 4096)) + 1) // 2)


def declip(audio: Tensor, audio_len: Tensor, flags: Optional[Tensor], rail_mode: int, rail: float, rail_ratio: float, min_run: int,
           order: int, iterations: int, out: Optional[dict] = None) -> dict:
    """ispk_declip_f64, four launches, no host read: the clipped samples (include/ispk.h has the definition) of fp32 audio [B, S]
    (unit stride on S, any row stride) with int64 lengths [B], restored by AR interpolation in float64 -> a dict of audio fp32
    [B, S] (any row stride, no memory of the input's), the DECLIP_OUTPUTS [B] each, and work (uint8 scratch of
    declip_workspace_bytes).  flags: the screen's int32 [B] or None; an item without bit 1 is copied.  `out` may hold any of the
    tensors; the rest is allocated."""
    B, S = _segment_audio(audio)
    if S > CONDITION_MAX_SAMPLES:
        raise ValueError(f"audio: at most {CONDITION_MAX_SAMPLES} samples an item, got {tuple(audio.shape)}")
    for name, v, top in (("min_run", min_run, DECLIP_MAX_RUN), ("order", order, DECLIP_MAX_ORDER), ("iterations", iterations, DECLIP_MAX_ITERATIONS)):
        if int(v) != v or not 1 <= v <= top:
            raise ValueError(f"{name} is an integer in [1, {top}], got {v!r}")
    dev = audio.device
    r = {}
    o = None if out is None else out.get("audio")
    o = torch.empty((B, S), dtype=torch.float32, device=dev) if o is None else o
    if o.dtype != torch.float32 or tuple(o.shape) != (B, S) or (S > 1 and o.stride(1) != 1) or (B > 1 and o.stride(0) < S):
        raise ValueError(f"out audio: fp32 [{B}, {S}] with unit stride on the samples, got {o.dtype} {tuple(o.shape)} strides {tuple(o.stride())}")
    ld_in, ld_out = (audio.stride(0) if B > 1 else max(audio.stride(0), S)), (o.stride(0) if B > 1 else max(o.stride(0), S))
    if B and S:
        a0, o0 = audio.data_ptr(), o.data_ptr()
        a1, o1 = a0 + 4 * ((B - 1) * ld_in + S), o0 + 4 * ((B - 1) * ld_out + S)
        if not (a1 <= o0 or o1 <= a0):
            raise ValueError("out audio overlaps the input: the declipper works out of place only (neighbouring windows read each "
                             "other's clipped values)")
    r["audio"] = o
    for name, dt, last in DECLIP_OUTPUTS:
        r.update(_segment_tensors(((name, dt, 0),), (B, last) if last else (B,), out, dev))
    need = declip_workspace_bytes(B, S)
    work = None if out is None else out.get("work")
    work = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev) if work is None else work
    if work.dtype != torch.uint8 or work.ndim != 1 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"work: contiguous uint8 of at least {need} bytes, got {work.dtype} {tuple(work.shape)}")
    if audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous():
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    if flags is not None and (flags.dtype != torch.int32 or flags.shape != (B,) or not flags.is_contiguous()):
        raise ValueError(f"flags: contiguous int32 [{B}], got {flags.dtype} {tuple(flags.shape)}")
    _rt._dev(audio, audio_len, flags, work, *r.values())
    # one read for the peak, one read and one write by the segments; per solved window and pass a banded Cholesky of <= 256 x 33
    _rt._launch("declip_kernels", 0.0, 12.0 * B * S, _rt.lib().ispk_declip_f64, audio.data_ptr(), ld_in, audio_len.data_ptr(), _rt._ptr(flags),
                int(rail_mode), float(rail), float(rail_ratio), int(min_run), int(order), int(iterations), o.data_ptr(), ld_out,
                *(r[name].data_ptr() for name, _, _ in DECLIP_OUTPUTS), work.data_ptr(), work.numel(), B, S, _rt._stream())
    r["work"] = work
    return r


# ------------------------------------------------------------------------------------------------------ noise reducer
NOISE_TILE_SAMPLES = 4096    # ispk_noise_tile_samples(): output samples of one item per workgroup of the reduce
NOISE_BINS = 513
NOISE_MIN_SAMPLES = 513       # below this the reflect padding is undefined: flagged short, copied
NOISE_MAX_GUARD = 65536       # frames
NOISE_MAX_SMOOTH_FRAMES, NOISE_MAX_SMOOTH_BINS = 2, 8
NOISE_FLAGS = {"no_profile": 1, "short": 2}
# name, dtype, trailing dimension (0: none), in the order of ispk_noise_profile_f64's output pointers
NOISE_OUTPUTS = (("noise", torch.float64, NOISE_BINS), ("noise_frames", torch.int32, 0), ("frames", torch.int32, 0),
                 ("flags", torch.int32, 0))


def noise_workspace_bytes(B: int, S: int) -> int:
    """ispk_noise_workspace_bytes: per item the hop sums (float64 [NH]), two int32 [NH + 1], a float64 [513] partial per tile of 16
    frames (S // 4096 + 1 of them) and one word."""
    NH = max(1, -(-S // 256))
    return 8 * B * (NH + 2 * ((NH + 2) // 2) + NOISE_BINS * (S // 4096 + 1) + 1)


def noise_profile(audio: Tensor, audio_len: Tensor, tables: Tensor, factor: float, ref_mode: int, ref: float, guard: int,
                  min_noise_frames: int, out: Optional[dict] = None) -> dict:
    """ispk_noise_profile_f64, four launches, no host read: the noise spectrum of every item of fp32 audio [B, S] (unit stride on
    S, any row stride) with int64 lengths [B], from its own pauses (include/ispk.h has the definitions) -> a dict of noise float64
    [B, 513]; noise_frames, frames, flags int32 [B]; work (uint8 scratch of noise_workspace_bytes).  tables: fp32, W_2048 and the
    window in front (the denoiser's).  `out` may hold any of them; the rest is allocated."""
    B, S = _segment_audio(audio)
    if S > CONDITION_MAX_SAMPLES:
        raise ValueError(f"audio: at most {CONDITION_MAX_SAMPLES} samples an item, got {tuple(audio.shape)}")
    dev = audio.device
    r = {}
    for name, dt, last in NOISE_OUTPUTS:
        r.update(_segment_tensors(((name, dt, 0),), (B, last) if last else (B,), out, dev))
    need = noise_workspace_bytes(B, S)
    work = None if out is None else out.get("work")
    work = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev) if work is None else work
    if work.dtype != torch.uint8 or work.ndim != 1 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"work: contiguous uint8 of at least {need} bytes, got {work.dtype} {tuple(work.shape)}")
    if audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous():
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() < FEATURE_TABLE_HEAD:
        raise ValueError(f"tables: contiguous fp32 of at least {FEATURE_TABLE_HEAD} values, got {tables.dtype} {tuple(tables.shape)}")
    _rt._dev(audio, audio_len, tables, work, *r.values())
    # the audio is read for the hop sums and again by the tiles that hold a noise frame; per such frame one 512-point transform
    frames = B * (S // FEATURE_HOP + 1)
    _rt._launch("noise_profile_kernels", frames * (5.0 * 512 * 9 + 513 * 12), 8.0 * B * S + 16.0 * B * (S // 4096 + 1) * NOISE_BINS,
                _rt.lib().ispk_noise_profile_f64, audio.data_ptr(), audio.stride(0) if B > 1 else max(audio.stride(0), S),
                audio_len.data_ptr(), tables.data_ptr(), float(factor), int(ref_mode), float(ref), int(guard), int(min_noise_frames),
                *(r[name].data_ptr() for name, _, _ in NOISE_OUTPUTS), work.data_ptr(), work.numel(), B, S, _rt._stream())
    r["work"] = work
    return r


def noise_reduce(audio: Tensor, audio_len: Optional[Tensor], tables: Tensor, noise: Tensor, index: Optional[Tensor],
                 flags: Optional[Tensor], over: float, g_min: float, smooth_frames: int, smooth_bins: int,
                 out: Optional[Tensor] = None) -> Tensor:
    """ispk_noise_reduce_f32, one launch, no host read: fp32 audio [B, S] (unit stride on S, any row stride) with int64 lengths
    [B] (None: all S samples) -> out fp32 [B, S]: STFT (1024 / 256, periodic Hann, reflect-centred), the Wiener gain max(1 - over
    noise[k] / |X|^2, g_min) smoothed with triangular weights over smooth_frames frames and smooth_bins bins on either side, ISTFT;
    zeros from audio_len on.  noise float64 [P, 513]; item b takes row index[b] (int32 [B]; None: row b).  Items below 513
    samples, with bit 1 or 2 in flags (int32 [B], the profile's; None: none) or with a row outside [0, P) are copied.  Out of
    place only."""
    _rt._dev(audio, audio_len, tables, noise, index, flags, out)
    B, S = _segment_audio(audio)
    if audio_len is not None and (audio_len.dtype != torch.int64 or audio_len.shape != (B,) or not audio_len.is_contiguous()):
        raise ValueError(f"audio_len: contiguous int64 [{B}], got {audio_len.dtype} {tuple(audio_len.shape)}")
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() < FEATURE_TABLE_HEAD:
        raise ValueError(f"tables: contiguous fp32 of at least {FEATURE_TABLE_HEAD} values, got {tables.dtype} {tuple(tables.shape)}")
    if noise.dtype != torch.float64 or noise.ndim != 2 or noise.shape[1] != NOISE_BINS or noise.shape[0] < 1 or not noise.is_contiguous():
        raise ValueError(f"noise: contiguous float64 [P, {NOISE_BINS}] with P >= 1, got {noise.dtype} {tuple(noise.shape)}")
    for name, t in (("index", index), ("flags", flags)):
        if t is not None and (t.dtype != torch.int32 or t.shape != (B,) or not t.is_contiguous()):
            raise ValueError(f"{name}: contiguous int32 [{B}], got {t.dtype} {tuple(t.shape)}")
    if not (over >= 0.0 and over < float("inf")) or not 0.0 < g_min <= 1.0:
        raise ValueError(f"over >= 0 and finite, 0 < g_min <= 1, got {over!r}, {g_min!r}")
    if int(smooth_frames) != smooth_frames or not 0 <= smooth_frames <= NOISE_MAX_SMOOTH_FRAMES:
        raise ValueError(f"smooth_frames is an integer in [0, {NOISE_MAX_SMOOTH_FRAMES}], got {smooth_frames!r}")
    if int(smooth_bins) != smooth_bins or not 0 <= smooth_bins <= NOISE_MAX_SMOOTH_BINS:
        raise ValueError(f"smooth_bins is an integer in [0, {NOISE_MAX_SMOOTH_BINS}], got {smooth_bins!r}")
    out = torch.empty((B, S), dtype=torch.float32, device=audio.device) if out is None else out
    _out_like("out", out, torch.float32, (B, S))
    if B == 0 or S == 0:
        return out
    # per hop: (19 + 2 smooth_frames) / 16 forward and 19 / 16 inverse 512-point transforms, the gains and their smoothing
    taps = (2 * smooth_frames + 1) * (2 * smooth_bins + 1)
    _rt._launch("noise_reduce_kernel", B * S / 256.0 * ((38.0 + 2 * smooth_frames) / 16.0 * 5.0 * 512 * 9 + 19.0 / 16.0 * 513 * (40.0 + 2 * taps)),
                8.0 * B * S, _rt.lib().ispk_noise_reduce_f32, audio.data_ptr(), audio.stride(0) if B > 1 else max(audio.stride(0), S),
                _rt._ptr(audio_len), tables.data_ptr(), noise.data_ptr(), noise.shape[0], _rt._ptr(index), _rt._ptr(flags), float(over),
                float(g_min), int(smooth_frames), int(smooth_bins), out.data_ptr(), out.stride(0) if B > 1 else max(out.stride(0), S), B, S,
                _rt._stream())
    return out


# ------------------------------------------------------------------------------------------------------ time stretch
STRETCH_TILE_SAMPLES = 4096   # ispk_stretch_tile_samples(): output samples of one item per workgroup of the synthesis
STRETCH_BINS = 513
STRETCH_MIN_SAMPLES = 513     # below this the reflect padding is undefined: flagged short, copied
STRETCH_RATES = (0.5, 2.0)    # the ring of analysis spectra holds two rounds of four frames
STRETCH_FLAGS = {"short": 1, "truncated": 2, "bad_rate": 4}


def stretch_workspace_bytes(B: int, S: int, out_samples: int) -> int:
    """ispk_stretch_workspace_bytes: per item and output tile of 4,096 samples one float64 phasor row, re [513] then im [513]."""
    return 8 * B * max(1, -(-out_samples // STRETCH_TILE_SAMPLES)) * 2 * STRETCH_BINS


def stretch(audio: Tensor, audio_len: Tensor, tables: Tensor, rate, out: Tensor, out_len: Tensor, wanted: Tensor, flags: Tensor,
            work: Optional[Tensor] = None) -> Tensor:
    """ispk_stretch_f32, three launches, no host read: the phase vocoder (include/ispk.h has the definition) of fp32 audio [B, S]
    (unit stride on S, any row stride) with int64 lengths [B] at `rate` - a float in [0.5, 2], or a float64 [B] device tensor with
    one rate per item - into out fp32 [B, out_samples] (any row stride, not audio itself): round(n / rate) samples of each item,
    cut at out_samples, zeros behind.  out_len, wanted int64 [B]; flags int32 [B], bits STRETCH_FLAGS.  tables: fp32, W_2048 and
    the window in front (the denoiser's); work: uint8 scratch of stretch_workspace_bytes (None: allocated)."""
    B, S = _mono_batch(audio, audio_len)
    if out.ndim != 2:
        raise ValueError(f"out: fp32 [{B}, out_samples], got {tuple(out.shape)}")
    out_samples = out.shape[1]
    _out_like("out", out, torch.float32, (B, out_samples))
    if not 1 <= S or not 1 <= out_samples <= CONDITION_MAX_SAMPLES:
        raise ValueError(f"audio and out: between 1 and {CONDITION_MAX_SAMPLES} samples a row, got {S} and {out_samples}")
    if B > 1 and (audio.stride(0) < S or out.stride(0) < out_samples):
        raise ValueError(f"audio / out: rows overlap (row strides {audio.stride(0)}, {out.stride(0)} < {S}, {out_samples})")
    _out_like("out_len", out_len, torch.int64, (B,))
    _out_like("wanted", wanted, torch.int64, (B,))
    _out_like("flags", flags, torch.int32, (B,))
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() < FEATURE_TABLE_HEAD:
        raise ValueError(f"tables: contiguous fp32 of at least {FEATURE_TABLE_HEAD} values, got {tables.dtype} {tuple(tables.shape)}")
    rates = rate if isinstance(rate, Tensor) else None
    if rates is not None:
        _out_like("rate", rates, torch.float64, (B,))
        scalar = 1.0
    else:
        scalar = float(rate)
        if not STRETCH_RATES[0] <= scalar <= STRETCH_RATES[1]:
            raise ValueError(f"rate in [{STRETCH_RATES[0]}, {STRETCH_RATES[1]}], got {rate!r}")
    need = stretch_workspace_bytes(B, S, out_samples)
    work = torch.empty((max(need, 8),), dtype=torch.uint8, device=audio.device) if work is None else work
    if work.dtype != torch.uint8 or work.ndim != 1 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"work: contiguous uint8 of at least {need} bytes, got {work.dtype} {tuple(work.shape)}")
    _rt._dev(audio, audio_len, tables, rates, out, out_len, wanted, flags, work)
    if B == 0:
        return out
    # per output hop: up to 2 (19 / 16) max(rate, 1) forward and 19 / 16 inverse 512-point transforms; per (output frame, bin)
    # about 40 float64 operations in each of the two passes
    hops = B * (out_samples / 256.0 + 1)
    _rt._launch("stretch_kernels", hops * ((2.0 * 2.0 + 1.0) * 19.0 / 16.0 * 5.0 * 512 * 9 + 2.0 * STRETCH_BINS * 40.0),
                4.0 * B * (2.0 * S + out_samples) + 32.0 * B * (out_samples / 4096.0 + 1) * STRETCH_BINS, _rt.lib().ispk_stretch_f32,
                audio.data_ptr(), audio.stride(0) if B > 1 else max(audio.stride(0), S), audio_len.data_ptr(), tables.data_ptr(), scalar,
                _rt._ptr(rates), out.data_ptr(), out.stride(0) if B > 1 else max(out.stride(0), out_samples), out_samples,
                out_len.data_ptr(), wanted.data_ptr(), flags.data_ptr(), work.data_ptr(), work.numel(), B, S, _rt._stream())
    return out


# ------------------------------------------------------------------------------------------------------ pitch tracker
PYIN_THRESHOLDS = 100         # ISPK_PYIN_THRESHOLDS
PYIN_MAX_BINS = 1024          # ISPK_PYIN_MAX_BINS: voiced states
PYIN_MAX_TROUGHS = 512        # the Boltzmann pieces of the observation table
PYIN_TABLE_DOUBLES = 1326     # ISPK_PYIN_TABLE_DOUBLES: thr [100], prior [100], its running sum [101], e2 [512], inv [513]
PYIN_MAX_PERIOD = 1022        # lags of a 2,048-sample frame with a 1,024-sample window
PYIN_MAX_WIDTH = 127          # transition window: two codes per offset fit one backpointer byte
PYIN_FRAMES_PER_BLOCK = 8     # ispk_pyin_frames_per_block(): frames of one item per workgroup of the observation


def pyin_workspace_bytes(B: int, M: int, NB: int) -> int:
    """ispk_pyin_workspace_bytes: two float64 per (item, frame) and one backpointer byte per (item, frame, state), rounded up to 8."""
    return 16 * B * M + (2 * B * M * NB + 7) // 8 * 8


def pyin_observe(audio: Tensor, audio_len: Tensor, tables: Tensor, prior: Tensor, obs: Tensor, frames: Optional[Tensor],
                 min_period: int, max_period: int, sample_rate: float, f_min: float, bins_per_semitone: int) -> Tensor:
    """ispk_pyin_observe_f32, one launch, no host read: the pYIN observation rows (include/ispk.h has the definition) of fp32 audio
    [B, S] (unit stride on S, any row stride) with int64 lengths [B] into obs fp32 [B, M, NB] (contiguous, M at least
    feature_frames(S)), zeros past each item's frames; frames int64 [B] or None receives the frame counts.  tables: fp32, W_2048 in
    front (data.twiddles(), or an AcousticFeatures' tables); prior: float64 [PYIN_TABLE_DOUBLES] (data.pitch.observation_table)."""
    _rt._dev(audio, audio_len, tables, prior, obs, frames)
    if audio.dtype != torch.float32 or audio.ndim != 2 or (audio.shape[1] > 1 and audio.stride(1) != 1):
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    B, S = audio.shape
    _out_like("audio_len", audio_len, torch.int64, (B,))
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() < 4096:
        raise ValueError(f"tables: contiguous fp32 of at least 4096 values, got {tables.dtype} {tuple(tables.shape)}")
    if prior.dtype != torch.float64 or tuple(prior.shape) != (PYIN_TABLE_DOUBLES,) or not prior.is_contiguous():
        raise ValueError(f"prior: contiguous float64 [{PYIN_TABLE_DOUBLES}], got {prior.dtype} {tuple(prior.shape)}")
    if obs.dtype != torch.float32 or obs.ndim != 3 or obs.shape[0] != B or not obs.is_contiguous():
        raise ValueError(f"obs: contiguous fp32 [{B}, M, NB], got {obs.dtype} {tuple(obs.shape)}")
    M, NB = obs.shape[1], obs.shape[2]
    if M < _rt.feature_frames(S) or not 1 <= NB <= PYIN_MAX_BINS:
        raise ValueError(f"obs: at least {_rt.feature_frames(S)} frames and 1 .. {PYIN_MAX_BINS} bins, got {tuple(obs.shape)}")
    if frames is not None:
        _out_like("frames", frames, torch.int64, (B,))
    if B == 0 or M == 0:
        return obs
    # per frame three 1,024-point transforms (5 radix-4 passes of 256 butterflies, ~34 flops each) and about 100 float64 steps per
    # trough; the audio is read 2048 / 256 times over through the cache, once from memory
    _rt._launch("pyin_observe_kernel", B * M * (3.0 * 5 * 256 * 34 + 4.0 * 2048 * 6), 4.0 * B * S + 4.0 * B * M * NB,
                _rt.lib().ispk_pyin_observe_f32, audio.data_ptr(), audio.stride(0) if B > 1 else max(audio.stride(0), S),
                audio_len.data_ptr(), tables.data_ptr(), prior.data_ptr(), obs.data_ptr(), _rt._ptr(frames), B, S, M, NB, int(min_period),
                int(max_period), float(sample_rate), float(f_min), int(bins_per_semitone), _rt._stream())
    return obs


_PYIN_OUTPUTS = (("state", torch.int32), ("f0", torch.float32), ("voiced", torch.int32), ("voiced_prob", torch.float32))


def pyin_decode(obs: Tensor, obs_len: Optional[Tensor], trans: Tensor, width: int, f_min: float, bins_per_semitone: int,
                out: Optional[dict] = None, pitch_mean: float = 0.0, pitch_std: float = 1.0) -> dict:
    """ispk_pyin_decode_f64, one launch, no host read: the Viterbi path (include/ispk.h has the recursion) through obs - fp32
    [B, M, NB] voiced probabilities, or float64 [B, M, 2 NB] ready log-observations - over the first obs_len[b] frames (int64 [B];
    None: M each) -> a dict of state int32, f0 fp32, voiced int32, voiced_prob fp32 [B, M]; frames int64 [B]; log_prob float64 [B];
    work (uint8 scratch of pyin_workspace_bytes); and pitch fp32 [B, M] = (f0 - pitch_mean) / pitch_std where `out` holds one.
    trans: float64 [width + NB + 3] (data.pitch.transition_table).  `out` may hold any of them; the rest is allocated."""
    if obs.ndim != 3 or obs.dtype not in (torch.float32, torch.float64) or not obs.is_contiguous():
        raise ValueError(f"obs: contiguous fp32 [B, M, NB] or float64 [B, M, 2 NB], got {obs.dtype} {tuple(obs.shape)}")
    is_log = obs.dtype == torch.float64
    B, M = obs.shape[:2]
    if is_log and obs.shape[2] % 2:
        raise ValueError(f"obs: float64 log-observations hold 2 NB states, got {tuple(obs.shape)}")
    NB = obs.shape[2] // 2 if is_log else obs.shape[2]
    if not 1 <= NB <= PYIN_MAX_BINS:
        raise ValueError(f"obs: 1 .. {PYIN_MAX_BINS} bins, got {NB}")
    if int(width) != width or not 1 <= width <= PYIN_MAX_WIDTH or width % 2 == 0:
        raise ValueError(f"width is an odd integer in [1, {PYIN_MAX_WIDTH}], got {width!r}")
    if trans.dtype != torch.float64 or tuple(trans.shape) != (width + NB + 3,) or not trans.is_contiguous():
        raise ValueError(f"trans: contiguous float64 [{width + NB + 3}], got {trans.dtype} {tuple(trans.shape)}")
    if obs_len is not None:
        _out_like("obs_len", obs_len, torch.int64, (B,))
    dev = obs.device
    r = {}
    for name, dt in _PYIN_OUTPUTS:
        r.update(_segment_tensors(((name, dt, 0),), (B, M), out, dev))
    r.update(_segment_tensors((("frames", torch.int64, 0), ("log_prob", torch.float64, 0)), (B,), out, dev))
    pitch = None if out is None else out.get("pitch")
    if pitch is not None:
        _out_like("pitch", pitch, torch.float32, (B, M))
        if not pitch.is_contiguous():
            raise ValueError("pitch: contiguous fp32 [B, M]")
        if float(pitch_std) == 0.0:
            raise ValueError("pitch std is 0")
        r["pitch"] = pitch
    need = pyin_workspace_bytes(B, M, NB)
    work = None if out is None else out.get("work")
    work = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev) if work is None else work
    if work.dtype != torch.uint8 or work.ndim != 1 or not work.is_contiguous() or work.numel() < need:
        raise ValueError(f"work: contiguous uint8 of at least {need} bytes, got {work.dtype} {tuple(work.shape)}")
    r["work"] = work
    _rt._dev(obs, obs_len, trans, *r.values())
    if B == 0:
        return r
    # per (frame, bin) 2 x width float64 add-compare steps and one log; the rows are read once, a backpointer byte per state
    _rt._launch("pyin_decode_kernel", B * M * NB * (4.0 * width + 40.0), obs.element_size() * float(obs.numel()) + 2.0 * B * M * NB,
                _rt.lib().ispk_pyin_decode_f64, obs.data_ptr(), int(is_log), _rt._ptr(obs_len), trans.data_ptr(), int(width), float(f_min),
                int(bins_per_semitone), float(pitch_mean), float(pitch_std), r["state"].data_ptr(), r["f0"].data_ptr(),
                r["voiced"].data_ptr(), r["voiced_prob"].data_ptr(), _rt._ptr(pitch), r["frames"].data_ptr(), r["log_prob"].data_ptr(),
                work.data_ptr(), work.numel(), B, M, NB, _rt._stream())
    return r
