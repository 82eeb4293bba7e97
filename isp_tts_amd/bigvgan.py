"""BigVGAN generator (the base 22.05 kHz configuration and any geometry of the same family): mel spectrograms
[B, n_mels, T] -> waveforms.  A HiFi-GAN skeleton whose leaky-ReLUs are anti-aliased periodic activations; the mel is the one
`data.AcousticFeatures` extracts and the acoustic model predicts.  Same call surface as `vocoder.Vocoder` and
`hifigan.HifiGan`: vocoder(mel, mel_len) -> (audio, audio_len).

    x = conv_pre(mel)                                                    Conv1d(n_mels, C0, 7, padding 3)
    for stage i:  x = ups[i][0](x)                                       ConvTranspose1d(C_i, C_i / 2, k_i, u_i, (k_i - u_i) / 2)
                  x = mean_j resblocks[i J + j](x)
      AMPBlock "1", per dilation m:  x = x + convs2[m](A[2m+1](convs1[m](A[2m](x))))
      AMPBlock "2", per dilation m:  x = x + convs[m](A[m](x))
    x = conv_post(activation_post(x))                                    Conv1d(C_last, 1, 7, padding 3)
    audio = tanh(x) if use_tanh_at_final else clamp(x, -1, 1)

    A(x) = down2(snake(up2(x))):  2x kaiser-sinc upsampling, u + sin(al u)^2 / (B + 1e-9) per channel, 2x low-pass
    downsampling, replicate padding (include/ispk.h gives the closed form).  snakebeta: al = exp(alpha), B = exp(beta) (or the
    plain values without snake_logscale); snake: B = al.

Launches per call (the loop is generator.ConvStackGenerator's): ispk_vocoder_unfold + one GEMM (conv_pre), per stage one
ispk_hifigan_upsample, per convolution one ispk_snake_aa (csrc/bigvgan.hip) into a scratch tensor and one ispk_hifigan_conv
with slope 1 (bias / residual fused on store; the last convolution of each block adds itself times 1 / J into the stage's
sum), ispk_snake_aa for activation_post, then ispk_hifigan_post[_clamp]_f32.  Base: 2 + 4 + 72 + 72 + 1 + 1 = 152 launches.  No ATen compute op, no host read: with `out=`
buffers a call is capturable.

Batches: as HifiGan - utterance b is vocoded as if mel[b, :, :mel_len[b]] were run alone, bit for bit; audio_len =
hop_length mel_len, samples past it are 0, nothing past mel_len is read.

Channel counts are multiples of 32 up to 512 (the base model).  The 112M models start at 1536 channels: NotImplementedError.
"""
from __future__ import annotations

import math
from typing import Sequence

import torch
from torch import Tensor, nn

from . import runtime
from .generator import ConvStackGenerator

FILTER_TAPS = 12
ACTIVATIONS = ("snake", "snakebeta")


def kaiser_sinc_filter() -> Tensor:
    """The low-pass of the anti-aliased activation at ratio 2: the kaiser-windowed sinc with cutoff 0.25, half-width 0.3 and 12
    taps (attenuation A = 2.285 * 5 * pi * 1.2 + 7.95 > 50 dB, so beta = 0.1102 (A - 8.7)), float64 [12], normalised to sum 1."""
    A = 2.285 * (FILTER_TAPS // 2 - 1) * math.pi * 1.2 + 7.95
    j = torch.arange(FILTER_TAPS, dtype=torch.float64)
    f = 0.5 * torch.kaiser_window(FILTER_TAPS, periodic=False, beta=0.1102 * (A - 8.7), dtype=torch.float64) \
        * torch.sinc(0.5 * (j - (FILTER_TAPS - 1) / 2))
    return f / f.sum()


class _Snake(nn.Module):
    def __init__(self, C: int, beta: bool, logscale: bool):
        super().__init__()
        # the published initial values: exp(0) = 1 with logscale, 1 without
        self.alpha = nn.Parameter(torch.zeros(C) if logscale else torch.ones(C))
        if beta:
            self.beta = nn.Parameter(torch.zeros(C) if logscale else torch.ones(C))


class _Filter(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", kaiser_sinc_filter().float().reshape(1, 1, FILTER_TAPS))


class _DownSample(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = _Filter()


class _Activation1d(nn.Module):
    """Names as published: act.alpha [, act.beta], upsample.filter, downsample.lowpass.filter."""

    def __init__(self, C: int, beta: bool, logscale: bool):
        super().__init__()
        self.act = _Snake(C, beta, logscale)
        self.upsample = _Filter()
        self.downsample = _DownSample()


class _AMPBlock1(nn.Module):
    def __init__(self, C: int, k: int, dilations: Sequence[int], beta: bool, logscale: bool):
        super().__init__()
        self.convs1 = nn.ModuleList([nn.Conv1d(C, C, k, dilation=d, padding=(k - 1) * d // 2) for d in dilations])
        self.convs2 = nn.ModuleList([nn.Conv1d(C, C, k, padding=(k - 1) // 2) for _ in dilations])
        self.activations = nn.ModuleList([_Activation1d(C, beta, logscale) for _ in range(2 * len(dilations))])


class _AMPBlock2(nn.Module):
    def __init__(self, C: int, k: int, dilations: Sequence[int], beta: bool, logscale: bool):
        super().__init__()
        self.convs = nn.ModuleList([nn.Conv1d(C, C, k, dilation=d, padding=(k - 1) * d // 2) for d in dilations])
        self.activations = nn.ModuleList([_Activation1d(C, beta, logscale) for _ in dilations])


def _check_activation(activation, filter_size, up_ratio, down_ratio) -> None:
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f"activation {activation!r}: \"snake\" and \"snakebeta\" are built")
    if filter_size != FILTER_TAPS:
        raise NotImplementedError(f"anti-aliasing filter of {filter_size} taps: {FILTER_TAPS} taps are built")
    if up_ratio != 2 or down_ratio != 2:
        raise NotImplementedError(f"anti-aliasing up / down ratio {up_ratio} / {down_ratio}: 2 / 2 is built")


class BigVGan(ConvStackGenerator):
    """The BigVGAN generator on libispk kernels.  Parameters and buffers carry the official state-dict names (conv_pre,
    ups.{i}.0, resblocks.{n}.convs1 / convs2 / convs.{m}, resblocks.{n}.activations.{l}.act.alpha / beta, ...upsample.filter,
    ...downsample.lowpass.filter, activation_post.*, conv_post) with plain weight / bias, so a weight-norm-free official dict
    loads with load_state_dict(strict=True); from_state_dict / from_pretrained fold weight norm.  In bf16 compute the
    anti-aliased activations and the output layer stay fp32.

    vocoder = BigVGan.from_pretrained("bigvgan_generator.pt").to("cuda").eval()      # config.json beside it
    audio, audio_len = vocoder(mel, mel_len)        # mel fp32 / fp16 [B, n_mels, T] (any strides), mel_len int64 [B] or None
    audio = vocoder.infer(mel)                      # audio fp32 [B, hop_length T]
    """

    UP_KEY = "ups.{i}.0"
    KEY_PREFIXES = ("conv_pre.", "ups.", "resblocks.", "activation_post.", "conv_post.")
    SLOPE = 1.0
    CONV_READS_STAGE = False                     # it reads snake_aa(stage tensor) in the stage's scratch tensor

    def __init__(self, n_mels: int = 80, upsample_initial_channel: int = 512, upsample_rates: Sequence[int] = (8, 8, 2, 2),
                 upsample_kernel_sizes: Sequence[int] = (16, 16, 4, 4), resblock: str = "1",
                 resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                 resblock_dilation_sizes: Sequence[Sequence[int]] = ((1, 3, 5),) * 3, activation: str = "snakebeta",
                 snake_logscale: bool = True, use_bias_at_final: bool = True, use_tanh_at_final: bool = True,
                 filter_size: int = FILTER_TAPS, up_ratio: int = 2, down_ratio: int = 2):
        super().__init__(n_mels, upsample_initial_channel, upsample_rates, upsample_kernel_sizes, resblock,
                         resblock_kernel_sizes, resblock_dilation_sizes)
        _check_activation(activation, filter_size, up_ratio, down_ratio)
        self.activation, self.snake_logscale = activation, bool(snake_logscale)
        self.use_bias_at_final, self.use_tanh_at_final = bool(use_bias_at_final), bool(use_tanh_at_final)
        beta, block = activation == "snakebeta", _AMPBlock1 if self.resblock == "1" else _AMPBlock2
        C_last = self._stack(lambda C, k, D: block(C, k, D, beta, self.snake_logscale), nest_ups=True)
        self.activation_post = _Activation1d(C_last, beta, self.snake_logscale)
        self.conv_post = nn.Conv1d(C_last, 1, 7, padding=3, bias=self.use_bias_at_final)

    def config(self) -> dict:
        return dict(super().config(), activation=self.activation, snake_logscale=self.snake_logscale,
                    use_bias_at_final=self.use_bias_at_final, use_tanh_at_final=self.use_tanh_at_final)

    @classmethod
    def _extra_args(cls, own: dict, cfg: dict) -> tuple:
        """Snake or snakebeta (is there an `act.beta`) and the filter length are read from names and shapes; snake_logscale,
        use_bias_at_final and use_tanh_at_final from the config, else the published defaults: logscale, bias and tanh.  The
        config's use_cuda_kernel is ignored."""
        if "activation_post.act.alpha" not in own:
            raise ValueError("missing keys: activation_post.act.alpha")
        activation = "snakebeta" if "activation_post.act.beta" in own else "snake"
        for k, t in own.items():
            if k.endswith(".filter") and t.shape[-1] != FILTER_TAPS:
                _check_activation(activation, int(t.shape[-1]), 2, 2)
        if "activation" in cfg and cfg["activation"] != activation:
            if cfg["activation"] not in ACTIVATIONS:
                _check_activation(cfg["activation"], FILTER_TAPS, 2, 2)
            raise ValueError(f"config does not fit the weights: activation {cfg['activation']!r}, weights give {activation!r}")
        use_bias = bool(cfg.get("use_bias_at_final", True))
        if not use_bias and "conv_post.bias" in own:
            raise ValueError("config does not fit the weights: use_bias_at_final false, weights have conv_post.bias")
        return (activation, bool(cfg.get("snake_logscale", True)), use_bias, bool(cfg.get("use_tanh_at_final", True)),
                int(cfg.get("filter_size", FILTER_TAPS)), int(cfg.get("up_ratio", 2)), int(cfg.get("down_ratio", 2)))

    # ---- kernel-ready weight images
    def _act(self, a: _Activation1d) -> tuple[Tensor, Tensor, Tensor]:
        """(al, inv_b, taps): float64, rounded once to fp32."""
        al = a.act.alpha.detach().double()
        al = al.exp() if self.snake_logscale else al
        if self.activation == "snakebeta":
            be = a.act.beta.detach().double()
            be = be.exp() if self.snake_logscale else be
        else:
            be = al
        taps = torch.cat([a.upsample.filter.detach().flatten(), a.downsample.lowpass.filter.detach().flatten()])
        return al.float().contiguous(), (1.0 / (be + 1e-9)).float().contiguous(), taps.float().contiguous()

    def _stage_conv(self, block, l, image):
        return self._act(block.activations[l]), image

    def _build(self, dtype: torch.dtype) -> dict:
        with torch.no_grad():
            return dict(super()._build(dtype), post_act=self._act(self.activation_post))

    # ---- forward
    def _conv_input(self, src, Tl, staged, scratch, kw):
        a, (w, b) = staged
        return runtime.snake_aa(src, Tl, *a, out=scratch, **kw), w, b

    def _post(self, x, Tl, w, scratch, audio, audio_len, kw):
        runtime.hifigan_post(runtime.snake_aa(x, Tl, *w["post_act"], out=scratch, **kw), Tl, w["post_w"], w["post_b"], audio,
                             audio_len, slope=1.0, final_clamp=not self.use_tanh_at_final, **kw)


