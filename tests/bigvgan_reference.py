"""The BigVGAN generator as a float64 torch module on the CPU, written from the network's description (conv_pre; per stage a
ConvTranspose1d with no activation before it and the mean of J AMPBlocks; activation_post, conv_post, tanh or clamp), with its
own weight-norm folding.  The anti-aliased activation is the padded form: replicate-pad 5, grouped conv_transpose1d with stride
2 times 2, crop 15 on each side, snake, replicate-pad (5, 6), grouped conv1d with stride 2 - not the closed form the kernel
evaluates.  tests/test_gpu_bigvgan.py compares isp_tts_amd.bigvgan.BigVGan with it, utterance by utterance."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor


def fold(sd: dict) -> dict:
    """Plain float64 `weight` / `bias` from a state dict in any weight-norm form: w = g v / ||v||, norm over all dims but 0."""
    out = {}
    for k, t in sd.items():
        t = t.double()
        for g_suf, v_suf in ((".weight_g", ".weight_v"), (".parametrizations.weight.original0",
                                                          ".parametrizations.weight.original1")):
            if k.endswith(v_suf):
                g = sd[k[:-len(v_suf)] + g_suf].double()
                dims = tuple(range(1, t.ndim))
                out[k[:-len(v_suf)] + ".weight"] = g * t / t.pow(2).sum(dim=dims, keepdim=True).sqrt()
                break
            if k.endswith(g_suf):
                break
        else:
            out[k] = t
    return out


def kaiser_sinc_taps() -> Tensor:
    """The 12-tap kaiser-windowed sinc with cutoff 0.25 and half-width 0.3, float64, normalised to sum 1."""
    A = 2.285 * 5 * math.pi * 1.2 + 7.95
    beta = 0.1102 * (A - 8.7)
    j = torch.arange(12, dtype=torch.float64)
    f = 0.5 * torch.kaiser_window(12, periodic=False, beta=beta, dtype=torch.float64) * torch.sinc(0.5 * (j - 5.5))
    return f / f.sum()


def snake_aa(x: Tensor, al: Tensor, inv_b: Tensor, fu: Tensor, fd: Tensor) -> Tensor:
    """x [N, C, n] -> [N, C, n] in x's dtype; al, inv_b [C]; fu, fd [12]."""
    C = x.shape[1]
    u = F.pad(x, (5, 5), mode="replicate")
    u = 2 * F.conv_transpose1d(u, fu.reshape(1, 1, 12).expand(C, 1, 12), stride=2, groups=C)[..., 15:-15]
    a = u + inv_b[None, :, None] * torch.sin(al[None, :, None] * u) ** 2
    a = F.pad(a, (5, 6), mode="replicate")
    return F.conv1d(a, fd.reshape(1, 1, 12).expand(C, 1, 12), stride=2, groups=C)


class Generator(torch.nn.Module):
    def __init__(self, sd: dict, config: dict):
        super().__init__()
        self.w = {k: v for k, v in fold(sd).items()}
        self.rates = tuple(config["upsample_rates"])
        self.up_kernels = tuple(config["upsample_kernel_sizes"])
        self.resblock = str(config["resblock"])
        self.res_kernels = tuple(config["resblock_kernel_sizes"])
        self.res_dilations = tuple(tuple(D) for D in config["resblock_dilation_sizes"])
        self.snakebeta = config.get("activation", "snakebeta") == "snakebeta"
        self.logscale = bool(config.get("snake_logscale", True))
        self.use_tanh = bool(config.get("use_tanh_at_final", True))
        self.hop = 1
        for u in self.rates:
            self.hop *= u

    def act(self, x: Tensor, name: str) -> Tensor:
        w = self.w
        al = w[name + ".act.alpha"]
        al = al.exp() if self.logscale else al
        if self.snakebeta:
            be = w[name + ".act.beta"]
            be = be.exp() if self.logscale else be
        else:
            be = al
        return snake_aa(x, al, 1.0 / (be + 1e-9), w[name + ".upsample.filter"].flatten(),
                        w[name + ".downsample.lowpass.filter"].flatten())

    def forward(self, mel: Tensor, rnd=lambda t: t) -> Tensor:
        """mel float64 [B, n_mels, T] -> audio [B, hop T].  `rnd` is applied to the input and the weight of every convolution
        but conv_post (identity: the float64 network)."""
        w = self.w

        def conv(x, name, k, d=1):
            return F.conv1d(rnd(x), rnd(w[name + ".weight"]), w[name + ".bias"], dilation=d, padding=(k - 1) * d // 2)

        x = conv(mel, "conv_pre", 7)
        J = len(self.res_kernels)
        for i, (u, k) in enumerate(zip(self.rates, self.up_kernels)):
            x = F.conv_transpose1d(rnd(x), rnd(w[f"ups.{i}.0.weight"]), w[f"ups.{i}.0.bias"], stride=u, padding=(k - u) // 2)
            total = None
            for j, (r, D) in enumerate(zip(self.res_kernels, self.res_dilations)):
                n, y = i * J + j, x
                p = f"resblocks.{n}."
                for m, d in enumerate(D):
                    if self.resblock == "1":
                        t = conv(self.act(y, p + f"activations.{2 * m}"), p + f"convs1.{m}", r, d)
                        y = conv(self.act(t, p + f"activations.{2 * m + 1}"), p + f"convs2.{m}", r) + y
                    else:
                        y = conv(self.act(y, p + f"activations.{m}"), p + f"convs.{m}", r, d) + y
                total = y if total is None else total + y
            x = total / J
        x = F.conv1d(self.act(x, "activation_post"), w["conv_post.weight"], w.get("conv_post.bias"), padding=3)
        return (torch.tanh(x) if self.use_tanh else x.clamp(-1.0, 1.0))[:, 0]


def build(sd: dict, config: dict) -> Generator:
    return Generator(sd, config).eval()


def _bf(x: Tensor) -> Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


@torch.no_grad()
def forward_bf16_operands(m: Generator, mel: Tensor) -> Tensor:
    """m on mel with the input and the weight of every convolution but conv_post rounded to bf16, as the bf16 path stores
    them; the activations, sums, biases, residuals, conv_post and the final tanh / clamp stay float64."""
    return m(mel, _bf)


def run_batch(m: Generator, mel: Tensor, mel_len: Optional[Tensor], fn=None) -> Tensor:
    """Utterance by utterance (mel[b, :, :len_b] alone), padded with zeros to [B, hop T]: the batch semantics' reference."""
    fn = fn or (lambda mm, x: mm(x))
    B, _, T = mel.shape
    out = torch.zeros((B, m.hop * T), dtype=torch.float64)
    with torch.no_grad():
        for b in range(B):
            n = T if mel_len is None else int(mel_len[b])
            if 0 < n <= T:
                out[b, :m.hop * n] = fn(m, mel[b:b + 1, :, :n].double())[0]
    return out
