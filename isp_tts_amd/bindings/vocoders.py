"""Mel spectrograms to waveforms: the Vocos, HiFi-GAN and BigVGAN vocoders (csrc/vocoder.hip, csrc/hifigan.hip,
csrc/bigvgan.hip, csrc/istftnet.hip) with their denoiser (csrc/denoise.hip) and the Griffin-Lim mel inversion (csrc/griffinlim.hip)."""
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt
from .audio import _out_like

__all__ = ["VOCODER_HOP", "VOCODER_TABLE_FLOATS", "_lengths_ptr", "vocoder_unfold", "dwconv7_ln", "istft_head",
           "HIFIGAN_TILE_ROWS", "HIFIGAN_MAX_CHANNELS", "HIFIGAN_MAX_KERNEL", "HIFIGAN_MAX_DILATION", "_hifigan_rows",
           "hifigan_conv", "_hifigan_bn", "hifigan_upsample", "hifigan_post", "ISTFTNET_TILE_FRAMES", "ISTFTNET_N_FFTS",
           "istftnet_table", "istftnet_head", "SNAKE_AA_TILE_ROWS", "snake_aa",
           "DENOISE_TILE_SAMPLES", "DENOISE_N_FFT", "DENOISE_HOP", "DENOISE_TABLE_FLOATS", "denoise", "GRIFFINLIM_TILE_SAMPLES",
           "GRIFFINLIM_N_FFT", "GRIFFINLIM_HOP", "GRIFFINLIM_PAD", "GRIFFINLIM_STEP", "GRIFFINLIM_INIT", "mel_to_linear",
           "griffinlim_step", "griffinlim_fast_step", "griffinlim_error"]


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


# --------------------------------------------------------------------------------------------------- iSTFTNet vocoder
ISTFTNET_TILE_FRAMES = 128    # ispk_istftnet_tile_frames(): frames of one utterance per workgroup of the output layer
ISTFTNET_N_FFTS = (8, 12, 16, 20, 24, 28, 32)      # the built geometries; hop = n_fft / 4, window length n_fft


def istftnet_table(n_fft: int) -> Tensor:
    """The output layer's table, made in float64: cos(2 pi m / N) [N], sin(2 pi m / N) [N], hann[t] / N [N], hann[t]^2 [N]
    (hann periodic) as fp32 [4 N] on the CPU."""
    m = torch.arange(n_fft, dtype=torch.float64)
    a = 2.0 * torch.pi * m / n_fft
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    return torch.cat([torch.cos(a), torch.sin(a), win / n_fft, win * win]).to(torch.float32)


def istftnet_head(x: Tensor, T: int, weight: Tensor, bias: Tensor, table: Tensor, n_fft: int, hop: int, audio: Tensor,
                  audio_len: Optional[Tensor] = None, lengths: Optional[Tensor] = None, len_mul: int = 1, slope: float = 0.01,
                  phase_scale: float = 1.0) -> Tensor:
    """ispk_istftnet_head_f32, one launch: x fp32 [B*T, C] rows -> audio fp32 [B, S >= hop T] = istft(exp(y[:H + 1]) exp(i
    phase_scale sin(y[H + 1:]))) with y = conv7(ReflectionPad1d((1, 0))(leaky_relu(x, slope))), H = n_fft / 2, periodic Hann,
    center = True: hop n_b samples for the n_b = lengths[b] * len_mul valid rows of utterance b (n_b = 1 counts as 0), zeros from
    there on; audio_len int64 [B] = hop n_b.  weight fp32 [7, n_fft + 2, C] contiguous, bias fp32 [n_fft + 2], table
    istftnet_table(n_fft) on the device."""
    _rt._dev(x, weight, bias, table, audio, audio_len, lengths)
    _hifigan_rows(x, "x")
    if n_fft not in ISTFTNET_N_FFTS or hop * 4 != n_fft:
        raise NotImplementedError(f"n_fft {n_fft} hop {hop}: n_fft in {ISTFTNET_N_FFTS} with hop = n_fft / 4 is built")
    assert audio.dtype == torch.float32 and audio.ndim == 2 and (audio.stride(1) == 1 or audio.shape[1] <= 1)
    B, S = audio.shape
    C = x.shape[1]
    assert x.shape[0] == B * T and S >= hop * T
    assert weight.shape == (7, n_fft + 2, C) and weight.is_contiguous() and weight.dtype == torch.float32
    assert bias.dtype == torch.float32 and bias.shape == (n_fft + 2,) and bias.is_contiguous()
    assert table.dtype == torch.float32 and table.is_contiguous() and table.numel() >= 4 * n_fft
    assert audio_len is None or (audio_len.dtype == torch.int64 and audio_len.shape == (B,) and audio_len.is_contiguous())
    ln = _lengths_ptr(lengths, B)
    if B == 0:
        return audio
    R = B * T
    _rt._launch(f"istftnet_head_kernel<{n_fft}>", R * (14.0 * C * (n_fft + 2) + 2.0 * n_fft * n_fft),
                float(R * C * 4 + B * S * 4), _rt.lib().ispk_istftnet_head_f32, x.data_ptr(), x.stride(0), weight.data_ptr(),
                bias.data_ptr(), table.data_ptr(), table.numel(), ln, len_mul, audio.data_ptr(), max(audio.stride(0), S),
                _rt._ptr(audio_len), B, T, S, C, n_fft, hop, slope, phase_scale, _rt._stream())
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
