"""What the mel vocoders share.  `MelVocoder`: the call surface of anything that maps mel spectrograms [B, n_mels, T] (+
mel_len) to (audio, audio_len) - `vocoder.Vocoder`, `hifigan.HifiGan`, `bigvgan.BigVGan`, `istftnet.IstftNet`.
`ConvStackGenerator`: the HiFi-GAN skeleton under the three GAN generators - geometry, loader, weight images and the stage /
block / unit loop on the kernels of csrc/hifigan.hip.  A generator adds its block containers and its output layer, and says,
per convolution, what the convolution reads.
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


class MelVocoder(nn.Module):
    """vocoder(mel, mel_len) -> (audio, audio_len), vocoder.infer(mel) -> audio.  A subclass has `_build(dtype)`, the
    kernel-ready images of its weights, and `_vocode(mel, mel_len, audio, audio_len)`, the launches for B, T > 0."""

    def __init__(self, n_mels: int, hop_length: int):
        super().__init__()
        self.n_mels, self.hop_length = n_mels, hop_length
        self.k_pad = (7 * n_mels + 7) // 8 * 8          # the first convolution's GEMM K: 7 n_mels padded to a multiple of 8
        self.compute_dtype = torch.float32
        self._cache = StagedWeights()

    def set_compute_dtype(self, dtype: torch.dtype) -> "MelVocoder":
        """fp32 (exact-fp32 MFMA) or bf16 (GEMM and convolution operands rounded to bf16, fp32 accumulation, fp32
        activations in memory; activation kernels, output layers and the ISTFT stay fp32)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError(f"compute dtype {dtype}: fp32 and bf16 are built")
        self.compute_dtype = dtype
        return self

    def staged(self, dtype: Optional[torch.dtype] = None) -> dict:
        """The kernel-ready images for `dtype` (default: the compute dtype), built once per dtype and rebuilt when a
        parameter or a buffer changes; build them before a graph capture (a warm-up call does)."""
        dtype = dtype or self.compute_dtype
        return self._cache.get(dtype, list(self.parameters()) + list(self.buffers()), lambda: self._build(dtype))

    def empty_outputs(self, B: int, T: int, device) -> tuple[Tensor, Tensor]:
        return (torch.empty((B, T * self.hop_length), dtype=torch.float32, device=device),
                torch.empty((B,), dtype=torch.int64, device=device))

    def forward(self, mel: Tensor, mel_len: Optional[Tensor] = None,
                out: Optional[tuple[Tensor, Tensor]] = None) -> tuple[Tensor, Tensor]:
        """mel fp32 / fp16 [B, n_mels, T] on the GPU -> (audio fp32 [B, S >= hop_length T], audio_len int64 [B])."""
        if not mel.is_cuda or (mel_len is not None and not mel_len.is_cuda):
            raise runtime.IspkError(f"{type(self).__name__} needs GPU tensors; there is no CPU fallback")
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
        self._vocode(mel, mel_len, audio, audio_len)
        return audio, audio_len

    @torch.no_grad()
    def infer(self, mel: Tensor) -> Tensor:
        """`vocoder.infer(mel)`: every utterance has all T frames; audio fp32 [B, hop_length T]."""
        return self.forward(mel)[0]


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


class ConvStackGenerator(MelVocoder):
    """conv_pre, per stage a transposed convolution and the mean of J residual blocks, conv_post.  Blocks of type "1" hold
    `convs1` / `convs2`, of type "2" `convs`, one entry per dilation.

    A subclass names its keys (UP_KEY, KEY_PREFIXES), gives the slope that `ispk_hifigan_conv` / `_upsample` fuse on load
    (SLOPE), builds its modules with `_stack` (conv_post after it), and has two steps of its own: `_conv_input`, what a
    convolution reads, and `_post`, the output layer.  CONV_READS_STAGE says which of the two `_conv_input` is: true when the
    convolution reads the stage tensor itself, so its halo forbids writing the unit's result over the unit's input; false when
    it reads a copy in a scratch tensor of the stage's size.  `head_hop`: the samples the output layer makes of one row of the
    last stage (1, or the hop of an inverse STFT), so hop_length = prod(upsample_rates) * head_hop."""

    UP_KEY = "ups.{i}"                           # the transposed convolution of stage i
    KEY_PREFIXES = ("conv_pre.", "ups.", "resblocks.", "conv_post.")
    TYPE2_DILATIONS = None                       # without a config; None: (1, 3, 5) for every block, as for type "1"
    SLOPE = 1.0
    CONV_READS_STAGE = True

    def __init__(self, n_mels: int, upsample_initial_channel: int, upsample_rates: Sequence[int],
                 upsample_kernel_sizes: Sequence[int], resblock: str, resblock_kernel_sizes: Sequence[int],
                 resblock_dilation_sizes: Sequence[Sequence[int]], head_hop: int = 1):
        rates, up_k = tuple(int(u) for u in upsample_rates), tuple(int(k) for k in upsample_kernel_sizes)
        res_k = tuple(int(k) for k in resblock_kernel_sizes)
        res_d = tuple(tuple(int(d) for d in D) for D in resblock_dilation_sizes)
        resblock = str(resblock)
        _check_geometry(n_mels, upsample_initial_channel, rates, up_k, resblock, res_k, res_d)
        super().__init__(n_mels, math.prod(rates) * head_hop)
        self.C0, self.rates, self.up_kernels = upsample_initial_channel, rates, up_k
        self.resblock, self.res_kernels, self.res_dilations = resblock, res_k, res_d

    def _stack(self, block, nest_ups: bool = False) -> int:
        """Registers conv_pre, ups and resblocks (`block(C, k, dilations)` each); -> conv_post's input channels."""
        C0 = self.C0
        self.conv_pre = nn.Conv1d(self.n_mels, C0, 7, padding=3)
        ups = [nn.ConvTranspose1d(C0 >> i, C0 >> (i + 1), k, u, padding=(k - u) // 2)
               for i, (u, k) in enumerate(zip(self.rates, self.up_kernels))]
        self.ups = nn.ModuleList([nn.ModuleList([up]) for up in ups] if nest_ups else ups)
        self.resblocks = nn.ModuleList([block(C0 >> (i + 1), k, D) for i in range(len(self.rates))
                                        for k, D in zip(self.res_kernels, self.res_dilations)])
        return C0 >> len(self.rates)

    def config(self) -> dict:
        return dict(n_mels=self.n_mels, upsample_initial_channel=self.C0, upsample_rates=self.rates,
                    upsample_kernel_sizes=self.up_kernels, resblock=self.resblock, resblock_kernel_sizes=self.res_kernels,
                    resblock_dilation_sizes=self.res_dilations)

    # ---- loading
    @classmethod
    def _extra_args(cls, own: dict, cfg: dict) -> tuple:
        """The constructor's arguments after the geometry, from the folded weights `own` and the config."""
        return ()

    @classmethod
    def from_state_dict(cls, sd: dict, config: Union[None, dict, str, os.PathLike] = None):
        """An official-layout generator state dict (or {"generator": ...} / {"state_dict": ...} around one) under any key
        prefix (found from `conv_pre`), weight norm in any of its three forms.  C0, n_mels, up-kernels, resblock type and
        resblock kernels are read from shapes and names; strides and dilations from `config` (a dict or the path of the official
        config.json), else the official defaults: stride = kernel / 2, dilations (1, 3, 5), or TYPE2_DILATIONS."""
        sd = _unwrap(sd)
        anchors = [k for k in sd if re.search(r"(^|\.)conv_pre\.(weight|weight_v|parametrizations\.weight\.original1)$", k)]
        if len(anchors) != 1:
            raise ValueError(f"missing keys: need exactly one '...conv_pre.weight[_v]', found {anchors}")
        prefix = anchors[0][:anchors[0].rindex("conv_pre.")]
        own = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        own = _fold_weight_norm({k: v for k, v in own.items() if k.startswith(cls.KEY_PREFIXES)})
        cfg = _load_config(config) or {}

        pre = own["conv_pre.weight"]
        if pre.ndim != 3 or pre.shape[2] != 7:
            raise NotImplementedError(f"conv_pre.weight {tuple(pre.shape)}: a kernel-7 Conv1d is built")
        C0, n_mels = int(pre.shape[0]), int(pre.shape[1])
        ups = sorted({int(m.group(1)) for k in own for m in [re.match(r"ups\.(\d+)\.", k)] if m})
        up_w = cls.UP_KEY + ".weight"
        if not ups or ups != list(range(len(ups))) or any(up_w.format(i=i) not in own for i in ups):
            raise ValueError(f"missing keys: ups.* numbered {ups}, need {up_w.format(i=0)} .. {up_w.format(i='n')}")
        up_k = tuple(int(own[up_w.format(i=i)].shape[2]) for i in ups)
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
        elif resblock == "2" and cls.TYPE2_DILATIONS is not None:
            res_d = cls.TYPE2_DILATIONS
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

        model = cls(n_mels, C0, rates, up_k, resblock, res_k, res_d, *cls._extra_args(own, cfg))
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
    def from_pretrained(cls, path, config: Union[None, dict, str, os.PathLike] = None):
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

    # ---- kernel-ready weight images
    def _stage_conv(self, block: nn.Module, l: int, image: tuple):
        """What `_conv_input` gets for the l-th convolution of `block` (in the order they run): its (weight, bias) image."""
        return image

    def _build(self, dtype: torch.dtype) -> dict:
        def conv(c: nn.Conv1d):             # [C_out, C_in, k] -> [k, C_out, C_in]
            return c.weight.detach().float().permute(2, 0, 1).to(dtype).contiguous(), c.bias.detach().float().contiguous()

        with torch.no_grad():
            pre = self.conv_pre.weight.detach().float().permute(0, 2, 1).reshape(self.C0, 7 * self.n_mels)   # column j*C + c
            pre_w = torch.zeros((self.C0, self.k_pad), dtype=torch.float32, device=pre.device)
            pre_w[:, :7 * self.n_mels] = pre
            ups = [self.get_submodule(self.UP_KEY.format(i=i)) for i in range(len(self.rates))]
            ups = [(u.weight.detach().float().permute(2, 1, 0).to(dtype).contiguous(), u.bias.detach().float().contiguous())
                   for u in ups]            # [C_in, C_out, k] -> [k, C_out, C_in]
            blocks = []
            for rb in self.resblocks:
                units = zip(rb.convs1, rb.convs2) if self.resblock == "1" else zip(rb.convs)
                blocks.append([tuple(self._stage_conv(rb, len(unit) * m + n, conv(c)) for n, c in enumerate(unit))
                               for m, unit in enumerate(units)])
            post_b = (self.conv_post.bias.detach().float().contiguous() if self.conv_post.bias is not None
                      else torch.zeros((1,), dtype=torch.float32, device=pre.device))
            return {"pre_w": pre_w.to(dtype).contiguous(), "pre_b": self.conv_pre.bias.detach().float().contiguous(),
                    "ups": ups, "blocks": blocks,
                    "post_w": self.conv_post.weight.detach().float()[0].t().contiguous(), "post_b": post_b}

    # ---- forward
    def _conv_input(self, src: Tensor, Tl: int, staged, scratch: Optional[Tensor], kw: dict) -> tuple[Tensor, Tensor, Tensor]:
        """(x, weight, bias) of one `ispk_hifigan_conv`: x is `src` (CONV_READS_STAGE) or made from it in `scratch`."""
        raise NotImplementedError

    def _post(self, x: Tensor, Tl: int, w: dict, scratch: Optional[Tensor], audio: Tensor, audio_len: Tensor, kw: dict) -> None:
        """The output layer on the last stage's sum x; `scratch` is that stage's."""
        raise NotImplementedError

    def _vocode(self, mel: Tensor, mel_len: Optional[Tensor], audio: Tensor, audio_len: Tensor) -> None:
        (B, _, T), cd = mel.shape, self.compute_dtype
        w = self.staged(cd)
        rows = torch.empty((B * T, self.k_pad), dtype=cd, device=mel.device)
        runtime.vocoder_unfold(mel, mel_len, rows)
        x = runtime.gemm(rows, w["pre_w"], bias=w["pre_b"], out_dtype=torch.float32)
        J, Tl, mul, slope = len(self.res_kernels), T, 1, self.SLOPE
        pair, conv_input = self.resblock == "1", self._conv_input
        for i, (u, ku) in enumerate(zip(self.rates, self.up_kernels)):
            up_w, up_b = w["ups"][i]
            xu = runtime.hifigan_upsample(x, Tl, up_w, up_b, ku, u, slope, lengths=mel_len, len_mul=mul)
            Tl, mul = Tl * u, mul * u
            total, keep = torch.empty_like(xu), torch.empty_like(xu)
            scratch = None if self.CONV_READS_STAGE else torch.empty_like(xu)
            # a pair's first result goes to `tmp`; a lone convolution that reads the stage tensor needs a second place too
            tmp = torch.empty_like(xu) if pair or self.CONV_READS_STAGE else None
            kw = dict(lengths=mel_len, len_mul=mul)
            for j, (k, D) in enumerate(zip(self.res_kernels, self.res_dilations)):
                units = w["blocks"][i * J + j]
                cur = xu
                for m, d in enumerate(D):
                    # the last convolution of a block adds itself times 1 / J into the stage's sum
                    fin = dict(out=total, accumulate=j > 0, scale=1.0 / J) if m == len(D) - 1 else None
                    if pair:
                        x1, w1, b1 = conv_input(cur, Tl, units[m][0], scratch, kw)
                        runtime.hifigan_conv(x1, Tl, w1, b1, k, d, slope, out=tmp, **kw)
                        x2, w2, b2 = conv_input(tmp, Tl, units[m][1], scratch, kw)
                        # the residual is read at the element that is written: x_{m+1} may replace x_m in `keep`
                        runtime.hifigan_conv(x2, Tl, w2, b2, k, 1, slope, resid=cur, **(fin or dict(out=keep)), **kw)
                        cur = keep
                    else:
                        x1, w1, b1 = conv_input(cur, Tl, units[m][0], scratch, kw)
                        # the input's halo is read: in place only when the convolution reads `scratch`
                        nxt = tmp if cur is keep and tmp is not None else keep
                        runtime.hifigan_conv(x1, Tl, w1, b1, k, d, slope, resid=cur, **(fin or dict(out=nxt)), **kw)
                        cur = nxt
            x = total
        self._post(x, Tl, w, scratch, audio, audio_len, kw)
