"""The HiFi-GAN generator as a float64 torch module on the CPU, written from the network's description (conv_pre; per stage
leaky-ReLU 0.1, ConvTranspose1d, the mean of J ResBlocks; leaky-ReLU 0.01, conv_post, tanh), with its own weight-norm folding.
tests/test_gpu_hifigan.py compares isp_tts_amd.hifigan.HifiGan with it, utterance by utterance."""
from __future__ import annotations

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


class Generator(torch.nn.Module):
    def __init__(self, sd: dict, config: dict):
        super().__init__()
        self.w = {k: v for k, v in fold(sd).items()}
        self.rates = tuple(config["upsample_rates"])
        self.up_kernels = tuple(config["upsample_kernel_sizes"])
        self.resblock = str(config["resblock"])
        self.res_kernels = tuple(config["resblock_kernel_sizes"])
        self.res_dilations = tuple(tuple(D) for D in config["resblock_dilation_sizes"])
        self.hop = 1
        for u in self.rates:
            self.hop *= u

    def forward(self, mel: Tensor, rnd=lambda t: t) -> Tensor:
        """mel float64 [B, n_mels, T] -> audio [B, hop T].  `rnd` is applied to the input and the weight of every convolution
        but conv_post (identity: the float64 network)."""
        w = self.w

        def conv(x, name, k, d=1):
            return F.conv1d(rnd(x), rnd(w[name + ".weight"]), w[name + ".bias"], dilation=d, padding=(k - 1) * d // 2)

        x = conv(mel, "conv_pre", 7)
        J = len(self.res_kernels)
        for i, (u, k) in enumerate(zip(self.rates, self.up_kernels)):
            x = F.conv_transpose1d(rnd(F.leaky_relu(x, 0.1)), rnd(w[f"ups.{i}.weight"]), w[f"ups.{i}.bias"], stride=u,
                                   padding=(k - u) // 2)
            total = None
            for j, (r, D) in enumerate(zip(self.res_kernels, self.res_dilations)):
                n, y = i * J + j, x
                for m, d in enumerate(D):
                    if self.resblock == "1":
                        t = conv(F.leaky_relu(y, 0.1), f"resblocks.{n}.convs1.{m}", r, d)
                        y = conv(F.leaky_relu(t, 0.1), f"resblocks.{n}.convs2.{m}", r) + y
                    else:
                        y = conv(F.leaky_relu(y, 0.1), f"resblocks.{n}.convs.{m}", r, d) + y
                total = y if total is None else total + y
            x = total / J
        x = F.conv1d(F.leaky_relu(x, 0.01), w["conv_post.weight"], w["conv_post.bias"], padding=3)
        return torch.tanh(x)[:, 0]


def build(sd: dict, config: dict) -> Generator:
    return Generator(sd, config).eval()


def _bf(x: Tensor) -> Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


@torch.no_grad()
def forward_bf16_operands(m: Generator, mel: Tensor) -> Tensor:
    """m on mel with the input (after its leaky-ReLU) and the weight of every convolution rounded to bf16, as the bf16 path
    stores them; sums, biases, residuals, conv_post and tanh stay float64."""
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
