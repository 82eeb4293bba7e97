"""A plain-torch restatement of the Vocos mel vocoder (VocosBackbone + ISTFTHead, padding "same") in the official module tree,
for the vocoder tests: run in float64 on the CPU it is the reference; `torch.jit.script` of it gives a TorchScript file
shaped like the notebook's vocos_ms_fp16.pts.  `forward_bf16_operands` is the same network with every GEMM operand (and the
bf16 hidden rows the kernels store) rounded to bf16, the reference of the bf16 bound."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn


class ConvNeXtBlock(nn.Module):
    def __init__(self, dim: int, intermediate_dim: int, gamma: bool):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, intermediate_dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(intermediate_dim, dim)
        self.gamma = nn.Parameter(torch.ones(dim)) if gamma else None

    def forward(self, x: Tensor) -> Tensor:
        residual = x
        x = self.dwconv(x).transpose(1, 2)
        x = self.pwconv2(self.act(self.pwconv1(self.norm(x))))
        if self.gamma is not None:
            x = self.gamma * x
        return residual + x.transpose(1, 2)


class VocosBackbone(nn.Module):
    def __init__(self, n_mels: int, dim: int, intermediate_dim: int, num_layers: int, gamma: bool = True):
        super().__init__()
        self.embed = nn.Conv1d(n_mels, dim, kernel_size=7, padding=3)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.convnext = nn.ModuleList([ConvNeXtBlock(dim, intermediate_dim, gamma) for _ in range(num_layers)])
        self.final_layer_norm = nn.LayerNorm(dim, eps=1e-6)

    def forward(self, x: Tensor) -> Tensor:
        x = self.embed(x)
        x = self.norm(x.transpose(1, 2)).transpose(1, 2)
        for blk in self.convnext:
            x = blk(x)
        return self.final_layer_norm(x.transpose(1, 2))            # [B, T, dim]


class ISTFT(nn.Module):
    """padding="same": irfft, window, overlap-add (F.fold), divide by the overlap-added window^2, trim (n_fft - hop) / 2."""

    def __init__(self, n_fft: int = 1024, hop_length: int = 256):
        super().__init__()
        self.n_fft, self.hop_length, self.pad = n_fft, hop_length, (n_fft - hop_length) // 2
        self.register_buffer("window", torch.hann_window(n_fft))

    def forward(self, spec: Tensor) -> Tensor:                     # complex [B, n_fft / 2 + 1, T]
        T = spec.shape[-1]
        frames = torch.fft.irfft(spec, self.n_fft, dim=1, norm="backward") * self.window[None, :, None]
        size = (T - 1) * self.hop_length + self.n_fft
        y = F.fold(frames, output_size=(1, size), kernel_size=(1, self.n_fft), stride=(1, self.hop_length))
        y = y[:, 0, 0, self.pad:size - self.pad]
        wsq = self.window.square().expand(1, T, -1).transpose(1, 2)
        env = F.fold(wsq, output_size=(1, size), kernel_size=(1, self.n_fft), stride=(1, self.hop_length))
        return y / env[0, 0, 0, self.pad:size - self.pad]


class ISTFTHead(nn.Module):
    def __init__(self, dim: int, n_fft: int = 1024, hop_length: int = 256):
        super().__init__()
        self.out = nn.Linear(dim, n_fft + 2)
        self.istft = ISTFT(n_fft, hop_length)

    def forward(self, x: Tensor) -> Tensor:
        return self.spectrum_to_audio(self.out(x).transpose(1, 2))

    def spectrum_to_audio(self, h: Tensor) -> Tensor:              # [B, n_fft + 2, T]: log-magnitudes, then phases
        mag, p = h.chunk(2, dim=1)
        mag = torch.clip(torch.exp(mag), max=1e2)
        return self.istft(torch.complex(mag * torch.cos(p), mag * torch.sin(p)))


class FeatureExtractorStub(nn.Module):
    """Stands for Vocos's MelSpectrogramFeatures: only its buffer matters (the loader must ignore feature_extractor.*)."""

    def __init__(self):
        super().__init__()
        self.register_buffer("window", torch.hann_window(1024))


class Vocos(nn.Module):
    def __init__(self, n_mels: int = 100, dim: int = 512, intermediate_dim: int = 1536, num_layers: int = 8,
                 gamma: bool = True):
        super().__init__()
        self.feature_extractor = FeatureExtractorStub()
        self.backbone = VocosBackbone(n_mels, dim, intermediate_dim, num_layers, gamma)
        self.head = ISTFTHead(dim)

    def forward(self, mel: Tensor) -> Tensor:
        return self.head(self.backbone(mel))

    @torch.jit.export
    def infer(self, mel: Tensor) -> Tensor:
        return self.forward(mel)


def build(sd: dict, dtype: torch.dtype = torch.float64) -> Vocos:
    """The module holding an official-layout state dict (backbone.*, head.*), in `dtype`, on the CPU."""
    emb = sd["backbone.embed.weight"]
    layers = len({k.split(".")[2] for k in sd if k.startswith("backbone.convnext.")})
    m = Vocos(emb.shape[1], emb.shape[0], sd["backbone.convnext.0.pwconv1.weight"].shape[0], layers,
              "backbone.convnext.0.gamma" in sd)
    full = dict(m.state_dict())
    full.update(sd)
    m.load_state_dict(full, strict=True)
    return m.to(dtype).eval()


def _bf(x: Tensor) -> Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


@torch.no_grad()
def forward_bf16_operands(m: Vocos, mel: Tensor) -> Tensor:
    """m (float64) on mel [B, C, T] with the operands of every GEMM rounded to bf16 as the bf16 path stores them: the
    unfolded mel and the embedding weight, each LayerNorm output that feeds a GEMM, pwconv1 / (gamma-folded) pwconv2 / head
    weights, the GELU output.  Sums, residual stream, LayerNorms and the ISTFT stay float64."""
    bb = m.backbone
    x = F.conv1d(_bf(mel.to(m.head.out.weight.dtype)), _bf(bb.embed.weight), bb.embed.bias, padding=3)
    x = bb.norm(x.transpose(1, 2))                                              # [B, T, dim], float64
    for blk in bb.convnext:
        y = F.conv1d(x.transpose(1, 2), blk.dwconv.weight, blk.dwconv.bias, padding=3, groups=x.shape[-1]).transpose(1, 2)
        y = _bf(blk.norm(y))
        hid = _bf(F.gelu(F.linear(y, _bf(blk.pwconv1.weight), blk.pwconv1.bias)))
        w2, b2 = blk.pwconv2.weight, blk.pwconv2.bias
        if blk.gamma is not None:
            w2, b2 = w2.float().mul(blk.gamma.float()[:, None]).to(w2.dtype), b2.float().mul(blk.gamma.float()).to(b2.dtype)
        x = x + F.linear(hid, _bf(w2), b2)
    y = _bf(bb.final_layer_norm(x))
    return m.head.spectrum_to_audio(F.linear(y, _bf(m.head.out.weight), m.head.out.bias).transpose(1, 2))


def run_batch(m: Vocos, mel: Tensor, mel_len: Optional[Tensor], fn=None) -> Tensor:
    """Utterance by utterance (mel[b, :, :len_b] alone), padded with zeros to [B, 256 T]: the batch semantics' reference."""
    fn = fn or (lambda mm, x: mm(x))
    B, _, T = mel.shape
    dt = m.head.out.weight.dtype
    out = torch.zeros((B, 256 * T), dtype=dt)
    with torch.no_grad():
        for b in range(B):
            n = T if mel_len is None else int(mel_len[b])
            if 0 < n <= T:
                out[b, :256 * n] = fn(m, mel[b:b + 1, :, :n].to(dt))[0]
    return out


def stft_same(x: Tensor, T: int, window: Tensor, n_fft: int = 1024, hop: int = 256) -> Tensor:
    """The analysis that ISTFT_same inverts: x zero-padded by (n_fft - hop) / 2 on the left (and as needed on the right),
    frame t starting at t hop - pad, windowed, rfft: complex [n_fft / 2 + 1, T]."""
    pad = (n_fft - hop) // 2
    need = (T - 1) * hop + n_fft
    xp = torch.zeros(need, dtype=x.dtype)
    n = min(x.shape[0], need - pad)
    xp[pad:pad + n] = x[:n]
    frames = xp.unfold(0, n_fft, hop)[:T] * window
    return torch.fft.rfft(frames, dim=1).T
