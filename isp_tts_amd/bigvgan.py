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

Launches per call: ispk_vocoder_unfold + one GEMM (conv_pre), per stage one ispk_hifigan_upsample, per convolution one
ispk_snake_aa (csrc/bigvgan.hip) into a scratch tensor and one ispk_hifigan_conv with slope 1 (bias / residual fused on store;
the last convolution of each block adds itself times 1 / J into the stage's sum), ispk_snake_aa for activation_post, then
ispk_hifigan_post[_clamp]_f32.  Base: 2 + 4 + 72 + 72 + 1 + 1 = 152 launches.  No ATen compute op, no host read: with `out=`
buffers a call is capturable.

Batches: as HifiGan - utterance b is vocoded as if mel[b, :, :mel_len[b]] were run alone, bit for bit; audio_len =
hop_length mel_len, samples past it are 0, nothing past mel_len is read.

Channel counts are multiples of 32 up to 512 (the base model).  The 112M models start at 1536 channels: NotImplementedError.
"""
from __future__ import annotations

import math
import os
import re
from typing import Optional, Sequence, Union

import torch
from torch import Tensor, nn

from . import runtime
from .hifigan import _check_geometry, _fold_weight_norm, _load_config, _unwrap
from .staging import StagedWeights

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


class BigVGan(nn.Module):
    """The BigVGAN generator on libispk kernels.  Parameters and buffers carry the official state-dict names (conv_pre,
    ups.{i}.0, resblocks.{n}.convs1 / convs2 / convs.{m}, resblocks.{n}.activations.{l}.act.alpha / beta, ...upsample.filter,
    ...downsample.lowpass.filter, activation_post.*, conv_post) with plain weight / bias, so a weight-norm-free official dict
    loads with load_state_dict(strict=True); from_state_dict / from_pretrained fold weight norm.

    vocoder = BigVGan.from_pretrained("bigvgan_generator.pt").to("cuda").eval()      # config.json beside it
    audio, audio_len = vocoder(mel, mel_len)        # mel fp32 / fp16 [B, n_mels, T] (any strides), mel_len int64 [B] or None
    audio = vocoder.infer(mel)                      # audio fp32 [B, hop_length T]
    """

    def __init__(self, n_mels: int = 80, upsample_initial_channel: int = 512, upsample_rates: Sequence[int] = (8, 8, 2, 2),
                 upsample_kernel_sizes: Sequence[int] = (16, 16, 4, 4), resblock: str = "1",
                 resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                 resblock_dilation_sizes: Sequence[Sequence[int]] = ((1, 3, 5),) * 3, activation: str = "snakebeta",
                 snake_logscale: bool = True, use_bias_at_final: bool = True, use_tanh_at_final: bool = True,
                 filter_size: int = FILTER_TAPS, up_ratio: int = 2, down_ratio: int = 2):
        super().__init__()
        rates, up_k = tuple(int(u) for u in upsample_rates), tuple(int(k) for k in upsample_kernel_sizes)
        res_k = tuple(int(k) for k in resblock_kernel_sizes)
        res_d = tuple(tuple(int(d) for d in D) for D in resblock_dilation_sizes)
        resblock = str(resblock)
        _check_geometry(n_mels, upsample_initial_channel, rates, up_k, resblock, res_k, res_d)
        _check_activation(activation, filter_size, up_ratio, down_ratio)
        self.n_mels, self.C0, self.rates, self.up_kernels = n_mels, upsample_initial_channel, rates, up_k
        self.resblock, self.res_kernels, self.res_dilations = resblock, res_k, res_d
        self.activation, self.snake_logscale = activation, bool(snake_logscale)
        self.use_bias_at_final, self.use_tanh_at_final = bool(use_bias_at_final), bool(use_tanh_at_final)
        self.hop_length = math.prod(rates)
        C0, beta = upsample_initial_channel, activation == "snakebeta"
        self.conv_pre = nn.Conv1d(n_mels, C0, 7, padding=3)
        self.ups = nn.ModuleList([nn.ModuleList([nn.ConvTranspose1d(C0 >> i, C0 >> (i + 1), k, u, padding=(k - u) // 2)])
                                  for i, (u, k) in enumerate(zip(rates, up_k))])
        block = _AMPBlock1 if resblock == "1" else _AMPBlock2
        self.resblocks = nn.ModuleList([block(C0 >> (i + 1), k, D, beta, self.snake_logscale)
                                        for i in range(len(rates)) for k, D in zip(res_k, res_d)])
        self.activation_post = _Activation1d(C0 >> len(rates), beta, self.snake_logscale)
        self.conv_post = nn.Conv1d(C0 >> len(rates), 1, 7, padding=3, bias=self.use_bias_at_final)
        self.k_pad = (7 * n_mels + 7) // 8 * 8          # conv_pre GEMM's K: 7 n_mels padded to a multiple of 8
        self.compute_dtype = torch.float32
        self._cache = StagedWeights()

    def config(self) -> dict:
        return dict(n_mels=self.n_mels, upsample_initial_channel=self.C0, upsample_rates=self.rates,
                    upsample_kernel_sizes=self.up_kernels, resblock=self.resblock, resblock_kernel_sizes=self.res_kernels,
                    resblock_dilation_sizes=self.res_dilations, activation=self.activation, snake_logscale=self.snake_logscale,
                    use_bias_at_final=self.use_bias_at_final, use_tanh_at_final=self.use_tanh_at_final)

    # ---- loading
    @classmethod
    def from_state_dict(cls, sd: dict, config: Union[None, dict, str, os.PathLike] = None) -> "BigVGan":
        """An official-layout generator state dict (or {"generator": ...} / {"state_dict": ...} around one) under any key
        prefix (found from `conv_pre`), weight norm in any of its three forms.  C0, n_mels, up-kernels, block type, block
        kernels, snake or snakebeta (is there an `act.beta`) and the filter length are read from shapes and names; strides,
        dilations, snake_logscale, use_bias_at_final and use_tanh_at_final from `config` (a dict or the path of the official
        config.json), else the published defaults: stride = kernel / 2, dilations (1, 3, 5), logscale, bias and tanh.  The
        config's use_cuda_kernel is ignored."""
        sd = _unwrap(sd)
        anchors = [k for k in sd if re.search(r"(^|\.)conv_pre\.(weight|weight_v|parametrizations\.weight\.original1)$", k)]
        if len(anchors) != 1:
            raise ValueError(f"missing keys: need exactly one '...conv_pre.weight[_v]', found {anchors}")
        prefix = anchors[0][:anchors[0].rindex("conv_pre.")]
        own = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        own = _fold_weight_norm({k: v for k, v in own.items()
                                 if k.startswith(("conv_pre.", "ups.", "resblocks.", "activation_post.", "conv_post."))})
        cfg = _load_config(config) or {}

        pre = own["conv_pre.weight"]
        if pre.ndim != 3 or pre.shape[2] != 7:
            raise NotImplementedError(f"conv_pre.weight {tuple(pre.shape)}: a kernel-7 Conv1d is built")
        C0, n_mels = int(pre.shape[0]), int(pre.shape[1])
        ups = sorted({int(m.group(1)) for k in own for m in [re.match(r"ups\.(\d+)\.", k)] if m})
        if not ups or ups != list(range(len(ups))) or any(f"ups.{i}.0.weight" not in own for i in ups):
            raise ValueError(f"missing keys: ups.* numbered {ups}, need ups.0.0.weight .. ups.n.0.weight")
        up_k = tuple(int(own[f"ups.{i}.0.weight"].shape[2]) for i in ups)
        blocks = sorted({int(m.group(1)) for k in own for m in [re.match(r"resblocks\.(\d+)\.", k)] if m})
        if not blocks or blocks != list(range(len(blocks))) or len(blocks) % len(ups) != 0:
            raise ValueError(f"missing keys: resblocks numbered {blocks} for {len(ups)} upsampling stages")
        J = len(blocks) // len(ups)
        if "resblocks.0.convs1.0.weight" in own:
            resblock, first = "1", "convs1"
        elif "resblocks.0.convs.0.weight" in own:
            resblock, first = "2", "convs"
        else:
            raise ValueError("missing keys: resblocks.0.convs1.0.weight or resblocks.0.convs.0.weight")
        missing = [f"resblocks.{j}.{first}.0.weight" for j in range(J) if f"resblocks.{j}.{first}.0.weight" not in own]
        if missing:
            raise ValueError(f"missing keys: {missing}")
        res_k = tuple(int(own[f"resblocks.{j}.{first}.0.weight"].shape[2]) for j in range(J))
        counts = [len({int(m.group(1)) for k in own for m in [re.match(rf"resblocks\.{j}\.{first}\.(\d+)\.", k)] if m})
                  for j in range(J)]
        if "activation_post.act.alpha" not in own:
            raise ValueError("missing keys: activation_post.act.alpha")
        activation = "snakebeta" if "activation_post.act.beta" in own else "snake"
        for k, t in own.items():
            if k.endswith(".filter") and t.shape[-1] != FILTER_TAPS:
                _check_activation(activation, int(t.shape[-1]), 2, 2)

        rates = tuple(cfg["upsample_rates"]) if "upsample_rates" in cfg else tuple(k // 2 for k in up_k)
        if "resblock_dilation_sizes" in cfg:
            res_d = tuple(tuple(D) for D in cfg["resblock_dilation_sizes"])
        else:
            res_d = ((1, 3, 5),) * J
        if len(rates) != len(ups) or len(res_d) != J or [len(D) for D in res_d] != counts:
            raise ValueError(f"config does not fit the weights: {len(ups)} stages, {J} resblocks per stage with {counts} "
                             f"convolutions, but upsample_rates {rates} and resblock_dilation_sizes {res_d}")
        for name, have in (("upsample_kernel_sizes", up_k), ("resblock_kernel_sizes", res_k)):
            if name in cfg and tuple(cfg[name]) != have:
                raise ValueError(f"config does not fit the weights: {name} {tuple(cfg[name])}, weights give {have}")
        if "resblock" in cfg and str(cfg["resblock"]) != resblock:
            raise ValueError(f"config does not fit the weights: resblock {cfg['resblock']!r}, weights give {resblock!r}")
        if "activation" in cfg and cfg["activation"] != activation:
            if cfg["activation"] not in ACTIVATIONS:
                _check_activation(cfg["activation"], FILTER_TAPS, 2, 2)
            raise ValueError(f"config does not fit the weights: activation {cfg['activation']!r}, weights give {activation!r}")
        use_bias = bool(cfg.get("use_bias_at_final", True))
        if not use_bias and "conv_post.bias" in own:
            raise ValueError("config does not fit the weights: use_bias_at_final false, weights have conv_post.bias")

        model = cls(n_mels, C0, rates, up_k, resblock, res_k, res_d, activation, bool(cfg.get("snake_logscale", True)), use_bias,
                    bool(cfg.get("use_tanh_at_final", True)), int(cfg.get("filter_size", FILTER_TAPS)),
                    int(cfg.get("up_ratio", 2)), int(cfg.get("down_ratio", 2)))
        expected = list(model.state_dict())
        missing = [k for k in expected if k not in own]
        if missing:
            raise ValueError(f"missing keys: {missing[:8]}{' ...' if len(missing) > 8 else ''}")
        for k, t in model.state_dict().items():
            if tuple(own[k].shape) != tuple(t.shape):
                raise ValueError(f"{k}: shape {tuple(own[k].shape)}, the geometry needs {tuple(t.shape)}")
        model.load_state_dict({k: own[k] for k in expected}, strict=True)
        return model

    @classmethod
    def from_pretrained(cls, path, config: Union[None, dict, str, os.PathLike] = None) -> "BigVGan":
        """A torch.save'd checkpoint: {"generator": state_dict} (the official files), {"state_dict": ...} or a bare state dict.
        Without `config`, a config.json beside the checkpoint is used if there is one."""
        obj = torch.load(path, map_location="cpu", weights_only=True)
        sd = _unwrap(obj)
        if not isinstance(sd, dict):
            raise ValueError(f"{os.fspath(path)}: not a state dict or a {{'generator': ...}} / {{'state_dict': ...}} dict")
        if config is None:
            beside = os.path.join(os.path.dirname(os.path.abspath(os.fspath(path))), "config.json")
            if os.path.exists(beside):
                config = beside
        return cls.from_state_dict(sd, config)

    def set_compute_dtype(self, dtype: torch.dtype) -> "BigVGan":
        """fp32 (exact-fp32 MFMA) or bf16 (convolution operands rounded to bf16, fp32 accumulation, fp32 activations in memory;
        the anti-aliased activations and the output layer stay fp32)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"compute dtype {dtype}: fp32 and bf16 are built")
        self.compute_dtype = dtype
        return self

    # ---- kernel-ready weight images
    def _build(self, dtype: torch.dtype) -> dict:
        def conv(c: nn.Conv1d):             # [C_out, C_in, k] -> [k, C_out, C_in]
            return c.weight.detach().float().permute(2, 0, 1).to(dtype).contiguous(), c.bias.detach().float().contiguous()

        def act(a: _Activation1d):          # (al, inv_b, taps): float64, rounded once to fp32
            al = a.act.alpha.detach().double()
            al = al.exp() if self.snake_logscale else al
            if self.activation == "snakebeta":
                be = a.act.beta.detach().double()
                be = be.exp() if self.snake_logscale else be
            else:
                be = al
            taps = torch.cat([a.upsample.filter.detach().flatten(), a.downsample.lowpass.filter.detach().flatten()])
            return al.float().contiguous(), (1.0 / (be + 1e-9)).float().contiguous(), taps.float().contiguous()

        with torch.no_grad():
            pre = self.conv_pre.weight.detach().float().permute(0, 2, 1).reshape(self.C0, 7 * self.n_mels)   # column j*C + c
            pre_w = torch.zeros((self.C0, self.k_pad), dtype=torch.float32, device=pre.device)
            pre_w[:, :7 * self.n_mels] = pre
            ups = [(u[0].weight.detach().float().permute(2, 1, 0).to(dtype).contiguous(), u[0].bias.detach().float().contiguous())
                   for u in self.ups]       # [C_in, C_out, k] -> [k, C_out, C_in]
            if self.resblock == "1":
                blocks = [[((act(rb.activations[2 * m]), conv(c1)), (act(rb.activations[2 * m + 1]), conv(c2)))
                           for m, (c1, c2) in enumerate(zip(rb.convs1, rb.convs2))] for rb in self.resblocks]
            else:
                blocks = [[((act(rb.activations[m]), conv(c)),) for m, c in enumerate(rb.convs)] for rb in self.resblocks]
            post_b = (self.conv_post.bias.detach().float().contiguous() if self.conv_post.bias is not None
                      else torch.zeros((1,), dtype=torch.float32, device=pre.device))
            return {"pre_w": pre_w.to(dtype).contiguous(), "pre_b": self.conv_pre.bias.detach().float().contiguous(),
                    "ups": ups, "blocks": blocks, "post_act": act(self.activation_post),
                    "post_w": self.conv_post.weight.detach().float()[0].t().contiguous(), "post_b": post_b}

    def staged(self, dtype: Optional[torch.dtype] = None) -> dict:
        """The kernel-ready images for `dtype` (default: the compute dtype), built once per dtype and rebuilt when a
        parameter or a filter changes; build them before a graph capture (a warm-up call does)."""
        dtype = dtype or self.compute_dtype
        return self._cache.get(dtype, list(self.parameters()) + list(self.buffers()), lambda: self._build(dtype))

    # ---- forward
    def empty_outputs(self, B: int, T: int, device) -> tuple[Tensor, Tensor]:
        return (torch.empty((B, T * self.hop_length), dtype=torch.float32, device=device),
                torch.empty((B,), dtype=torch.int64, device=device))

    def forward(self, mel: Tensor, mel_len: Optional[Tensor] = None,
                out: Optional[tuple[Tensor, Tensor]] = None) -> tuple[Tensor, Tensor]:
        """mel fp32 / fp16 [B, n_mels, T] on the GPU -> (audio fp32 [B, S >= hop_length T], audio_len int64 [B])."""
        if not mel.is_cuda or (mel_len is not None and not mel_len.is_cuda):
            raise runtime.IspkError("BigVGan needs GPU tensors; there is no CPU fallback")
        if mel.ndim != 3 or mel.dtype not in (torch.float32, torch.float16) or mel.shape[1] != self.n_mels:
            raise ValueError(f"mel: fp32 / fp16 [B, {self.n_mels}, T], got {mel.dtype} {tuple(mel.shape)}")
        B, _, T = mel.shape
        audio, audio_len = out if out is not None else self.empty_outputs(B, T, mel.device)
        if B == 0:
            return audio, audio_len
        if T == 0:
            runtime.zero_(audio_len)
            if audio.numel():
                runtime.zero_(audio)
            return audio, audio_len
        cd, dev = self.compute_dtype, mel.device
        w = self.staged(cd)
        rows = torch.empty((B * T, self.k_pad), dtype=cd, device=dev)
        runtime.vocoder_unfold(mel, mel_len, rows)
        x = runtime.gemm(rows, w["pre_w"], bias=w["pre_b"], out_dtype=torch.float32)
        J, Tl, mul = len(self.res_kernels), T, 1
        for i, (u, ku) in enumerate(zip(self.rates, self.up_kernels)):
            up_w, up_b = w["ups"][i]
            xu = runtime.hifigan_upsample(x, Tl, up_w, up_b, ku, u, 1.0, lengths=mel_len, len_mul=mul)
            Tl, mul = Tl * u, mul * u
            total, keep, act = (torch.empty_like(xu) for _ in range(3))
            tmp = torch.empty_like(xu) if self.resblock == "1" else None
            kw = dict(lengths=mel_len, len_mul=mul)

            def snake(src, a):
                return runtime.snake_aa(src, Tl, *a, out=act, **kw)

            for j, (k, D) in enumerate(zip(self.res_kernels, self.res_dilations)):
                units = w["blocks"][i * J + j]
                cur = xu
                for m, d in enumerate(D):
                    last = m == len(D) - 1
                    fin = dict(out=total, accumulate=j > 0, scale=1.0 / J) if last else {}
                    if self.resblock == "1":
                        (a1, (w1, b1)), (a2, (w2, b2)) = units[m]
                        runtime.hifigan_conv(snake(cur, a1), Tl, w1, b1, k, d, out=tmp, **kw)
                        # the residual is read at the element that is written: x_{m+1} may replace x_m in `keep`
                        runtime.hifigan_conv(snake(tmp, a2), Tl, w2, b2, k, 1, resid=cur, **(fin or dict(out=keep)), **kw)
                        cur = keep
                    else:
                        ((a1, (w1, b1)),) = units[m]
                        # the convolution reads `act`, the residual at the element that is written: in place in `keep`
                        runtime.hifigan_conv(snake(cur, a1), Tl, w1, b1, k, d, resid=cur, **(fin or dict(out=keep)), **kw)
                        cur = keep
            x = total
        runtime.hifigan_post(runtime.snake_aa(x, Tl, *w["post_act"], out=act, lengths=mel_len, len_mul=mul), Tl, w["post_w"],
                             w["post_b"], audio, audio_len, lengths=mel_len, len_mul=mul, slope=1.0,
                             final_clamp=not self.use_tanh_at_final)
        return audio, audio_len

    @torch.no_grad()
    def infer(self, mel: Tensor) -> Tensor:
        """`vocoder.infer(mel)`: every utterance has all T frames; audio fp32 [B, hop_length T]."""
        return self.forward(mel)[0]
