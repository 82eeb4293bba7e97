"""HiFi-GAN generator (V1 / V3 and any geometry of the same family): mel spectrograms [B, n_mels, T] -> waveforms.  The mel it
was defined on (22,050 Hz, n_fft 1024, hop 256, 80 slaney mels, 0 - 8 kHz, log(clamp(x, 1e-5))) is the one
`data.AcousticFeatures` extracts and the acoustic model predicts, so a public 22.05 kHz generator vocodes `infer`'s output as
it is.  Same call surface as `vocoder.Vocoder`: vocoder(mel, mel_len) -> (audio, audio_len).

    x = conv_pre(mel)                                                    Conv1d(n_mels, C0, 7, padding 3)
    for stage i:  x = ups[i](leaky_relu(x, 0.1))                         ConvTranspose1d(C_i, C_i / 2, k_i, u_i, (k_i - u_i) / 2)
                  x = mean_j resblocks[i J + j](x)
      ResBlock "1", per dilation d:  x = x + conv2(leaky_relu(conv1_d(leaky_relu(x, 0.1)), 0.1))
      ResBlock "2", per dilation d:  x = x + conv_d(leaky_relu(x, 0.1))
    audio = tanh(conv_post(leaky_relu(x, 0.01)))                         Conv1d(C_last, 1, 7, padding 3)

Launches per call (csrc/hifigan.hip unless noted): ispk_vocoder_unfold + one GEMM (conv_pre), per stage one
ispk_hifigan_upsample and one ispk_hifigan_conv per convolution (leaky-ReLU fused on load, bias / residual fused on store; the
last convolution of each ResBlock adds itself times 1 / J into the stage's sum, so the mean needs no launch), then
ispk_hifigan_post_f32.  V1: 2 + 4 + 72 + 1 = 79 launches; V3: 2 + 3 + 18 + 1 = 24.  No ATen compute op, no host read: with
`out=` buffers a call is capturable.

Batches: utterance b is vocoded as if mel[b, :, :mel_len[b]] were run alone, bit for bit (a workgroup never spans two
utterances and every sum runs in an order fixed by the position inside the utterance); audio_len = hop_length mel_len, samples
past it are 0, nothing past mel_len is read.

Channel counts are multiples of 32 up to 512 (V1, V3).  V2 ends at 16 and 8 channels: NotImplementedError.
"""
from __future__ import annotations

import json
import math
import os
import re
from typing import Optional, Sequence, Union

import torch
from torch import Tensor, nn

from . import runtime
from .staging import StagedWeights

MAX_MELS = 128                                   # ispk_vocoder_unfold
LRELU_SLOPE, POST_SLOPE = 0.1, 0.01
V3_DILATIONS = ((1, 2), (2, 6), (3, 12))

CONFIGS = {
    "v1": dict(n_mels=80, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
               resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3),
    "v2": dict(n_mels=80, upsample_initial_channel=128, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
               resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3),
    "v3": dict(n_mels=80, upsample_initial_channel=256, upsample_rates=(8, 8, 4), upsample_kernel_sizes=(16, 16, 8),
               resblock="2", resblock_kernel_sizes=(3, 5, 7), resblock_dilation_sizes=V3_DILATIONS),
}


class _ResBlock1(nn.Module):
    def __init__(self, C: int, k: int, dilations: Sequence[int]):
        super().__init__()
        self.convs1 = nn.ModuleList([nn.Conv1d(C, C, k, dilation=d, padding=(k - 1) * d // 2) for d in dilations])
        self.convs2 = nn.ModuleList([nn.Conv1d(C, C, k, padding=(k - 1) // 2) for _ in dilations])


class _ResBlock2(nn.Module):
    def __init__(self, C: int, k: int, dilations: Sequence[int]):
        super().__init__()
        self.convs = nn.ModuleList([nn.Conv1d(C, C, k, dilation=d, padding=(k - 1) * d // 2) for d in dilations])


def _check_geometry(n_mels, C0, rates, up_kernels, resblock, res_kernels, res_dilations) -> None:
    if str(resblock) not in ("1", "2"):
        raise NotImplementedError(f"resblock {resblock!r}: types \"1\" and \"2\" are built")
    if not 1 <= n_mels <= MAX_MELS:
        raise NotImplementedError(f"n_mels {n_mels}: 1 .. {MAX_MELS} mel channels are built")
    if len(rates) == 0 or len(rates) != len(up_kernels):
        raise ValueError(f"upsample_rates {tuple(rates)} and upsample_kernel_sizes {tuple(up_kernels)} differ in length")
    if len(res_kernels) == 0 or len(res_kernels) != len(res_dilations):
        raise ValueError(f"resblock_kernel_sizes {tuple(res_kernels)} and resblock_dilation_sizes differ in length")
    if C0 % (1 << len(rates)) != 0:
        raise NotImplementedError(f"upsample_initial_channel {C0} does not halve {len(rates)} times")
    for i in range(len(rates) + 1):
        C = C0 >> i
        if C % 32 != 0 or not 32 <= C <= runtime.HIFIGAN_MAX_CHANNELS:
            raise NotImplementedError(f"channel count {C} (stage {i} of upsample_initial_channel {C0}): multiples of 32 up to "
                                      f"{runtime.HIFIGAN_MAX_CHANNELS} are built")
    for k, u in zip(up_kernels, rates):
        if u < 1 or u > 64 or k < u or k > 128 or (k - u) % 2 != 0:
            raise NotImplementedError(f"ConvTranspose1d kernel {k} stride {u}: k >= stride with k - stride even is built")
    for k, D in zip(res_kernels, res_dilations):
        if k % 2 != 1 or not 1 <= k <= runtime.HIFIGAN_MAX_KERNEL:
            raise NotImplementedError(f"resblock kernel {k}: odd kernels up to {runtime.HIFIGAN_MAX_KERNEL} are built")
        if len(D) == 0:
            raise ValueError("a resblock needs at least one dilation")
        for d in D:
            if not 1 <= d <= runtime.HIFIGAN_MAX_DILATION:
                raise NotImplementedError(f"dilation {d}: 1 .. {runtime.HIFIGAN_MAX_DILATION} are built")


def _fold_weight_norm(own: dict) -> dict:
    """Plain `weight` / `bias` tensors from any of the three forms of a weight-normalised convolution: w = g v / ||v||, the norm
    over all dims but dim 0 (C_out of a Conv1d, C_in of a ConvTranspose1d), in float64."""
    out = {}
    forms = ((".weight_g", ".weight_v"), (".parametrizations.weight.original0", ".parametrizations.weight.original1"))
    for key, t in own.items():
        for g_suf, v_suf in forms:
            if key.endswith(v_suf):
                base = key[:-len(v_suf)]
                if base + g_suf not in own:
                    raise ValueError(f"missing keys: {base + g_suf}")
                g, v = own[base + g_suf].detach().double(), t.detach().double()
                norm = v.pow(2).sum(dim=tuple(range(1, v.ndim)), keepdim=True).sqrt()
                out[base + ".weight"] = (g.reshape(norm.shape) * v / norm).to(torch.float32)
                break
            if key.endswith(g_suf):
                if key[:-len(g_suf)] + v_suf not in own:
                    raise ValueError(f"missing keys: {key[:-len(g_suf)] + v_suf}")
                break
        else:
            out[key] = t.detach().to(torch.float32)
    return out


def _unwrap(obj):
    if isinstance(obj, dict):
        for k in ("generator", "state_dict"):
            if k in obj and isinstance(obj[k], dict):
                return obj[k]
    return obj


def _load_config(config) -> Optional[dict]:
    if config is None or isinstance(config, dict):
        return config
    with open(config) as f:
        return json.load(f)


class HifiGan(nn.Module):
    """The HiFi-GAN generator on libispk kernels.  Parameters carry the official state-dict names (conv_pre, ups.{i},
    resblocks.{n}.convs1 / convs2 / convs.{m}, conv_post) with plain weight / bias, so a weight-norm-free official dict loads
    with load_state_dict(strict=True); from_state_dict / from_pretrained fold weight norm.

    vocoder = HifiGan.from_pretrained("generator_v1", "config.json").to("cuda").eval()
    audio, audio_len = vocoder(mel, mel_len)        # mel fp32 / fp16 [B, n_mels, T] (any strides), mel_len int64 [B] or None
    audio = vocoder.infer(mel)                      # audio fp32 [B, hop_length T]
    """

    def __init__(self, n_mels: int = 80, upsample_initial_channel: int = 512, upsample_rates: Sequence[int] = (8, 8, 2, 2),
                 upsample_kernel_sizes: Sequence[int] = (16, 16, 4, 4), resblock: str = "1",
                 resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                 resblock_dilation_sizes: Sequence[Sequence[int]] = ((1, 3, 5),) * 3):
        super().__init__()
        rates, up_k = tuple(int(u) for u in upsample_rates), tuple(int(k) for k in upsample_kernel_sizes)
        res_k = tuple(int(k) for k in resblock_kernel_sizes)
        res_d = tuple(tuple(int(d) for d in D) for D in resblock_dilation_sizes)
        resblock = str(resblock)
        _check_geometry(n_mels, upsample_initial_channel, rates, up_k, resblock, res_k, res_d)
        self.n_mels, self.C0, self.rates, self.up_kernels = n_mels, upsample_initial_channel, rates, up_k
        self.resblock, self.res_kernels, self.res_dilations = resblock, res_k, res_d
        self.hop_length = math.prod(rates)
        C0 = upsample_initial_channel
        self.conv_pre = nn.Conv1d(n_mels, C0, 7, padding=3)
        self.ups = nn.ModuleList([nn.ConvTranspose1d(C0 >> i, C0 >> (i + 1), k, u, padding=(k - u) // 2)
                                  for i, (u, k) in enumerate(zip(rates, up_k))])
        block = _ResBlock1 if resblock == "1" else _ResBlock2
        self.resblocks = nn.ModuleList([block(C0 >> (i + 1), k, D) for i in range(len(rates)) for k, D in zip(res_k, res_d)])
        self.conv_post = nn.Conv1d(C0 >> len(rates), 1, 7, padding=3)
        self.k_pad = (7 * n_mels + 7) // 8 * 8          # conv_pre GEMM's K: 7 n_mels padded to a multiple of 8
        self.compute_dtype = torch.float32
        self._cache = StagedWeights()

    def config(self) -> dict:
        return dict(n_mels=self.n_mels, upsample_initial_channel=self.C0, upsample_rates=self.rates,
                    upsample_kernel_sizes=self.up_kernels, resblock=self.resblock, resblock_kernel_sizes=self.res_kernels,
                    resblock_dilation_sizes=self.res_dilations)

    # ---- loading
    @classmethod
    def from_state_dict(cls, sd: dict, config: Union[None, dict, str, os.PathLike] = None) -> "HifiGan":
        """An official-layout generator state dict (or {"generator": ...} / {"state_dict": ...} around one) under any key
        prefix (found from `conv_pre`), weight norm in any of its three forms.  C0, n_mels, up-kernels, resblock type and
        resblock kernels are read from shapes and names; strides and dilations from `config` (a dict or the path of the official
        config.json), else the official defaults: stride = kernel / 2, dilations (1, 3, 5) for type "1", the V3 table for "2"."""
        sd = _unwrap(sd)
        anchors = [k for k in sd if re.search(r"(^|\.)conv_pre\.(weight|weight_v|parametrizations\.weight\.original1)$", k)]
        if len(anchors) != 1:
            raise ValueError(f"missing keys: need exactly one '...conv_pre.weight[_v]', found {anchors}")
        prefix = anchors[0][:anchors[0].rindex("conv_pre.")]
        own = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        own = _fold_weight_norm({k: v for k, v in own.items() if k.startswith(("conv_pre.", "ups.", "resblocks.", "conv_post."))})
        cfg = _load_config(config) or {}

        pre = own["conv_pre.weight"]
        if pre.ndim != 3 or pre.shape[2] != 7:
            raise NotImplementedError(f"conv_pre.weight {tuple(pre.shape)}: a kernel-7 Conv1d is built")
        C0, n_mels = int(pre.shape[0]), int(pre.shape[1])
        ups = sorted({int(m.group(1)) for k in own for m in [re.match(r"ups\.(\d+)\.", k)] if m})
        if not ups or ups != list(range(len(ups))) or any(f"ups.{i}.weight" not in own for i in ups):
            raise ValueError(f"missing keys: ups.* numbered {ups}, need ups.0.weight .. ups.n.weight")
        up_k = tuple(int(own[f"ups.{i}.weight"].shape[2]) for i in ups)
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

        rates = tuple(cfg["upsample_rates"]) if "upsample_rates" in cfg else tuple(k // 2 for k in up_k)
        if "resblock_dilation_sizes" in cfg:
            res_d = tuple(tuple(D) for D in cfg["resblock_dilation_sizes"])
        elif resblock == "1":
            res_d = ((1, 3, 5),) * J
        else:
            res_d = V3_DILATIONS
        if len(rates) != len(ups) or len(res_d) != J or [len(D) for D in res_d] != counts:
            raise ValueError(f"config does not fit the weights: {len(ups)} stages, {J} resblocks per stage with {counts} "
                             f"convolutions, but upsample_rates {rates} and resblock_dilation_sizes {res_d}")
        for name, have in (("upsample_kernel_sizes", up_k), ("resblock_kernel_sizes", res_k)):
            if name in cfg and tuple(cfg[name]) != have:
                raise ValueError(f"config does not fit the weights: {name} {tuple(cfg[name])}, weights give {have}")
        if "resblock" in cfg and str(cfg["resblock"]) != resblock:
            raise ValueError(f"config does not fit the weights: resblock {cfg['resblock']!r}, weights give {resblock!r}")

        model = cls(n_mels, C0, rates, up_k, resblock, res_k, res_d)
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
    def from_pretrained(cls, path, config: Union[None, dict, str, os.PathLike] = None) -> "HifiGan":
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

    def set_compute_dtype(self, dtype: torch.dtype) -> "HifiGan":
        """fp32 (exact-fp32 MFMA) or bf16 (convolution operands rounded to bf16, fp32 accumulation, fp32 activations in memory;
        the output layer stays fp32)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"compute dtype {dtype}: fp32 and bf16 are built")
        self.compute_dtype = dtype
        return self

    # ---- kernel-ready weight images
    def _build(self, dtype: torch.dtype) -> dict:
        def conv(c: nn.Conv1d):             # [C_out, C_in, k] -> [k, C_out, C_in]
            return c.weight.detach().float().permute(2, 0, 1).to(dtype).contiguous(), c.bias.detach().float().contiguous()

        with torch.no_grad():
            pre = self.conv_pre.weight.detach().float().permute(0, 2, 1).reshape(self.C0, 7 * self.n_mels)   # column j*C + c
            pre_w = torch.zeros((self.C0, self.k_pad), dtype=torch.float32, device=pre.device)
            pre_w[:, :7 * self.n_mels] = pre
            ups = [(u.weight.detach().float().permute(2, 1, 0).to(dtype).contiguous(), u.bias.detach().float().contiguous())
                   for u in self.ups]       # [C_in, C_out, k] -> [k, C_out, C_in]
            if self.resblock == "1":
                blocks = [[(conv(c1), conv(c2)) for c1, c2 in zip(rb.convs1, rb.convs2)] for rb in self.resblocks]
            else:
                blocks = [[(conv(c),) for c in rb.convs] for rb in self.resblocks]
            return {"pre_w": pre_w.to(dtype).contiguous(), "pre_b": self.conv_pre.bias.detach().float().contiguous(),
                    "ups": ups, "blocks": blocks,
                    "post_w": self.conv_post.weight.detach().float()[0].t().contiguous(),
                    "post_b": self.conv_post.bias.detach().float().contiguous()}

    def staged(self, dtype: Optional[torch.dtype] = None) -> dict:
        """The kernel-ready images for `dtype` (default: the compute dtype), built once per dtype and rebuilt when a
        parameter changes; build them before a graph capture (a warm-up call does)."""
        dtype = dtype or self.compute_dtype
        return self._cache.get(dtype, list(self.parameters()), lambda: self._build(dtype))

    # ---- forward
    def empty_outputs(self, B: int, T: int, device) -> tuple[Tensor, Tensor]:
        return (torch.empty((B, T * self.hop_length), dtype=torch.float32, device=device),
                torch.empty((B,), dtype=torch.int64, device=device))

    def forward(self, mel: Tensor, mel_len: Optional[Tensor] = None,
                out: Optional[tuple[Tensor, Tensor]] = None) -> tuple[Tensor, Tensor]:
        """mel fp32 / fp16 [B, n_mels, T] on the GPU -> (audio fp32 [B, S >= hop_length T], audio_len int64 [B])."""
        if not mel.is_cuda or (mel_len is not None and not mel_len.is_cuda):
            raise runtime.IspkError("HifiGan needs GPU tensors; there is no CPU fallback")
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
            xu = runtime.hifigan_upsample(x, Tl, up_w, up_b, ku, u, LRELU_SLOPE, lengths=mel_len, len_mul=mul)
            Tl, mul = Tl * u, mul * u
            total, tmp, keep = torch.empty_like(xu), torch.empty_like(xu), torch.empty_like(xu)
            kw = dict(slope=LRELU_SLOPE, lengths=mel_len, len_mul=mul)
            for j, (k, D) in enumerate(zip(self.res_kernels, self.res_dilations)):
                units = w["blocks"][i * J + j]
                cur = xu
                for m, d in enumerate(D):
                    last = m == len(D) - 1
                    fin = dict(out=total, accumulate=j > 0, scale=1.0 / J) if last else {}
                    if self.resblock == "1":
                        (w1, b1), (w2, b2) = units[m]
                        runtime.hifigan_conv(cur, Tl, w1, b1, k, d, out=tmp, **kw)
                        # the residual is read at the element that is written: x_{m+1} may replace x_m in `keep`
                        runtime.hifigan_conv(tmp, Tl, w2, b2, k, 1, resid=cur, **(fin or dict(out=keep)), **kw)
                        cur = keep
                    else:
                        ((w1, b1),) = units[m]
                        nxt = keep if cur is not keep else tmp       # the input's halo is read: never in place
                        runtime.hifigan_conv(cur, Tl, w1, b1, k, d, resid=cur, **(fin or dict(out=nxt)), **kw)
                        cur = nxt
            x = total
        runtime.hifigan_post(x, Tl, w["post_w"], w["post_b"], audio, audio_len, lengths=mel_len, len_mul=mul, slope=POST_SLOPE)
        return audio, audio_len

    @torch.no_grad()
    def infer(self, mel: Tensor) -> Tensor:
        """`vocoder.infer(mel)`: every utterance has all T frames; audio fp32 [B, hop_length T]."""
        return self.forward(mel)[0]
