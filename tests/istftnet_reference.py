"""The iSTFTNet generator as a float64 torch module on the CPU, written from the network's description (conv_pre; per stage
leaky-ReLU 0.1, ConvTranspose1d, the mean of J ResBlocks; leaky-ReLU 0.01, ReflectionPad1d((1, 0)), conv_post, exp on the first
n_fft / 2 + 1 channels, phase_scale * sin on the rest, torch.istft with a periodic Hann window, center = True), with
hifigan_reference's weight-norm folding.  tests/test_gpu_istftnet.py compares isp_tts_amd.istftnet.IstftNet with it, utterance
by utterance; tests/test_istftnet_host.py checks its inverse STFT against a literal numpy restatement (`istft_literal`)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from hifigan_reference import fold


def head(y: Tensor, n_fft: int, hop: int, phase_scale: float = 1.0) -> Tensor:
    """conv_post's output y float64 [B, n_fft + 2, F] -> audio [B, hop (F - 1)]."""
    H = n_fft // 2
    spec = torch.exp(y[:, :H + 1]) * torch.exp(1j * (phase_scale * torch.sin(y[:, H + 1:])))
    return torch.istft(spec, n_fft, hop, n_fft, torch.hann_window(n_fft, periodic=True, dtype=torch.float64), center=True)


def post(x: Tensor, weight: Tensor, bias: Tensor, n_fft: int, hop: int, phase_scale: float = 1.0, slope: float = 0.01,
         want_y: bool = False):
    """The output layer on the last stage's x float64 [B, C, R], R >= 2: leaky-ReLU, reflection pad, conv_post, `head`."""
    y = F.conv1d(F.pad(F.leaky_relu(x, slope), (1, 0), mode="reflect"), weight, bias, padding=3)
    return (head(y, n_fft, hop, phase_scale), y) if want_y else head(y, n_fft, hop, phase_scale)


def istft_literal(spec: np.ndarray, n_fft: int, hop: int) -> np.ndarray:
    """spec complex128 [n_fft / 2 + 1, F] -> float64 [hop (F - 1)]: the explicit inverse DFT sum of the Hermitian extension,
    a periodic Hann window, overlap-add, division by the sum of squared windows, trim of n_fft / 2 on both sides."""
    K, Fr = spec.shape
    assert K == n_fft // 2 + 1
    t = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * t / n_fft)
    full = np.zeros((n_fft, Fr), dtype=np.complex128)
    full[:K] = spec
    full[K:] = np.conj(spec[1:K - 1][::-1])
    out = np.zeros(n_fft + hop * (Fr - 1))
    env = np.zeros_like(out)
    for f in range(Fr):
        frame = np.zeros(n_fft)
        for k in range(n_fft):
            frame += (full[k, f] * np.exp(2j * np.pi * k * t / n_fft)).real
        out[f * hop:f * hop + n_fft] += win * frame / n_fft
        env[f * hop:f * hop + n_fft] += win * win
    H = n_fft // 2
    keep = slice(H, H + hop * (Fr - 1))             # the envelope is 0 at sample 0 (w[0] = 0), which the trim drops
    return out[keep] / env[keep]


class Generator(torch.nn.Module):
    def __init__(self, sd: dict, config: dict):
        super().__init__()
        self.w = {k: v for k, v in fold(sd).items()}
        self.rates = tuple(config["upsample_rates"])
        self.up_kernels = tuple(config["upsample_kernel_sizes"])
        self.resblock = str(config["resblock"])
        self.res_kernels = tuple(config["resblock_kernel_sizes"])
        self.res_dilations = tuple(tuple(D) for D in config["resblock_dilation_sizes"])
        self.n_fft = int(config.get("gen_istft_n_fft", 16))
        self.istft_hop = int(config.get("gen_istft_hop_size", self.n_fft // 4))
        self.phase_scale = float(config.get("phase_scale", 1.0))
        self.hop = self.istft_hop
        for u in self.rates:
            self.hop *= u

    def forward(self, mel: Tensor, rnd=lambda t: t, want_y: bool = False):
        """mel float64 [B, n_mels, T] -> audio [B, hop T].  `rnd` is applied to the input and the weight of every convolution
        but conv_post (identity: the float64 network).  want_y: (audio, conv_post's output [B, n_fft + 2, F])."""
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
        return post(x, w["conv_post.weight"], w["conv_post.bias"], self.n_fft, self.istft_hop, self.phase_scale, want_y=want_y)


def build(sd: dict, config: dict) -> Generator:
    return Generator(sd, config).eval()


def _bf(x: Tensor) -> Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


@torch.no_grad()
def forward_bf16_operands(m: Generator, mel: Tensor) -> Tensor:
    """m on mel with the input (after its leaky-ReLU) and the weight of every convolution but conv_post rounded to bf16, as
    the bf16 path stores them; sums, biases, residuals and the whole output layer stay float64."""
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
