"""Vocos vocoder, mel variant (VocosBackbone + ISTFTHead, padding "same"): mel spectrograms [B, n_mels, T] -> waveforms, the
last step of the reference's inference notebook (`mel2audio`: `vocoder.infer(mel)` of a TorchScript Vocos).

    x = LayerNorm(Conv1d(n_mels -> dim, 7, padding 3)(mel))
    for each ConvNeXt block: x = x + gamma * pwconv2(gelu(pwconv1(LayerNorm(dwconv7(x)))))
    h = head.out(LayerNorm(x));  mag = clip(exp(h[:513]), max=100);  audio = ISTFT_same(mag * exp(i h[513:]))

Launches per call (csrc/vocoder.hip for the three that are not a GEMM or a LayerNorm): ispk_vocoder_unfold (the embedding
convolution's GEMM rows and the row mask), the embedding GEMM + ispk_layernorm_f32, per block ispk_dwconv7_ln_f32 and two
GEMMs (GELU epilogue; bias + residual + row mask epilogue, gamma folded into pwconv2), the final LayerNorm, the head GEMM,
ispk_istft_head_f32.  No ATen compute op, no host read: with `out=` buffers a call is capturable.

Batches: utterance b is vocoded as if mel[b, :, :mel_len[b]] were run alone (every convolution and the ISTFT's overlap-add
and envelope see only its own frames); audio_len = 256 mel_len, samples past it are 0, nothing past mel_len is read.
"""
from __future__ import annotations

import io
import os
import re
from typing import Optional

import torch
from torch import Tensor, nn

from . import runtime
from .data.features import twiddles
from .generator import MAX_MELS, MelVocoder

N_FFT = 1024
HOP = runtime.VOCODER_HOP
EPS = 1e-6
MAX_DIM = 1024         # ispk_dwconv7_ln_f32 and ispk_layernorm_f32: dim % 64 == 0, dim <= 1024
INTER_MULTIPLE = 32    # pwconv1 rows: the GEMMs' N tiles
_HEAD_N = N_FFT + 8    # head.out rows padded with zero rows to 1032 (16-byte aligned fp32 rows)


class _Block(nn.Module):
    def __init__(self, dim: int, inter: int, gamma: bool):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=EPS)
        self.pwconv1 = nn.Linear(dim, inter)
        self.pwconv2 = nn.Linear(inter, dim)
        self.gamma = nn.Parameter(torch.ones(dim)) if gamma else None


class _Backbone(nn.Module):
    def __init__(self, n_mels: int, dim: int, inter: int, num_layers: int, gamma: bool):
        super().__init__()
        self.embed = nn.Conv1d(n_mels, dim, kernel_size=7, padding=3)
        self.norm = nn.LayerNorm(dim, eps=EPS)
        self.convnext = nn.ModuleList([_Block(dim, inter, gamma) for _ in range(num_layers)])
        self.final_layer_norm = nn.LayerNorm(dim, eps=EPS)


class _ISTFT(nn.Module):
    def __init__(self, n_fft: int):
        super().__init__()
        self.register_buffer("window", torch.hann_window(n_fft))


class _Head(nn.Module):
    def __init__(self, dim: int, n_fft: int):
        super().__init__()
        self.out = nn.Linear(dim, n_fft + 2)
        self.istft = _ISTFT(n_fft)


def _check_dims(n_mels: int, dim: int, inter: int, n_fft: int, window: int, hop_length: int, padding: str) -> None:
    if padding != "same":
        raise NotImplementedError(f"padding={padding!r}: only the \"same\" ISTFT padding is built")
    if n_fft != N_FFT or window != N_FFT:
        raise NotImplementedError(f"n_fft / win_length other than {N_FFT} are not built (head gives n_fft {n_fft}, window "
                                  f"{window})")
    if hop_length != HOP:
        raise NotImplementedError(f"hop_length other than {HOP} is not built")
    if dim % 64 != 0 or not 64 <= dim <= MAX_DIM:
        raise NotImplementedError(f"dim {dim}: a multiple of 64 up to {MAX_DIM} is built")
    if inter % INTER_MULTIPLE != 0 or inter <= 0:
        raise NotImplementedError(f"intermediate dim {inter}: a multiple of {INTER_MULTIPLE} is built")
    if not 1 <= n_mels <= MAX_MELS:
        raise NotImplementedError(f"n_mels {n_mels}: 1 .. {MAX_MELS} mel channels are built")


def _official_keys(num_layers: int, gamma: bool) -> list[str]:
    keys = ["backbone.embed.weight", "backbone.embed.bias", "backbone.norm.weight", "backbone.norm.bias"]
    for i in range(num_layers):
        p = f"backbone.convnext.{i}."
        keys += [p + k for k in ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias",
                                 "pwconv2.weight", "pwconv2.bias")]
        if gamma:
            keys.append(p + "gamma")
    return keys + ["backbone.final_layer_norm.weight", "backbone.final_layer_norm.bias", "head.out.weight", "head.out.bias",
                   "head.istft.window"]


class Vocoder(MelVocoder):
    """The Vocos mel vocoder on libispk kernels.  Parameters carry the official state-dict names (backbone.*, head.*), so an
    official-layout dict loads with load_state_dict(strict=True).  In bf16 compute the residual stream, the head output and
    the ISTFT stay fp32.

    vocoder = Vocoder.from_pretrained(path).to("cuda").eval()
    audio, audio_len = vocoder(mel, mel_len)        # mel fp32 / fp16 [B, n_mels, T] (any strides), mel_len int64 [B] or None
    audio = vocoder.infer(mel)                      # the notebook's call: audio fp32 [B, 256 T]
    """

    def __init__(self, n_mels: int = 100, dim: int = 512, inter: int = 1536, num_layers: int = 8, gamma: bool = True,
                 hop_length: int = HOP, padding: str = "same"):
        _check_dims(n_mels, dim, inter, N_FFT, N_FFT, hop_length, padding)
        super().__init__(n_mels, hop_length)
        self.dim, self.inter, self.num_layers, self.has_gamma, self.padding = dim, inter, num_layers, gamma, padding
        self.backbone = _Backbone(n_mels, dim, inter, num_layers, gamma)
        self.head = _Head(dim, N_FFT)

    # ---- loading
    @classmethod
    def from_state_dict(cls, sd: dict, hop_length: int = HOP, padding: str = "same") -> "Vocoder":
        """An official-layout state dict, under any common key prefix (found from `backbone.embed.weight`); other keys
        (feature_extractor.*) are ignored.  Dims are read from the shapes; fp16 weights are cast to fp32."""
        anchors = [k for k in sd if k.endswith("backbone.embed.weight")]
        if len(anchors) != 1:
            raise ValueError(f"missing keys: need exactly one '...backbone.embed.weight', found {anchors}")
        prefix = anchors[0][:-len("backbone.embed.weight")]
        own = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        own = {k: v for k, v in own.items() if k.startswith(("backbone.", "head."))}
        ada = [k for k in own if k.endswith(".norm.scale.weight")]
        if ada:
            raise NotImplementedError(f"AdaLayerNorm checkpoints (conditioned Vocos: {ada[0]}) are not built")
        emb = own["backbone.embed.weight"]
        if emb.ndim != 3 or emb.shape[2] != 7:
            raise NotImplementedError(f"backbone.embed.weight {tuple(emb.shape)}: a kernel-7 Conv1d is built")
        dim, n_mels = int(emb.shape[0]), int(emb.shape[1])
        layers = sorted({int(m.group(1)) for k in own for m in [re.match(r"backbone\.convnext\.(\d+)\.", k)] if m})
        num_layers = len(layers)
        if layers != list(range(num_layers)):
            raise ValueError(f"missing keys: ConvNeXt blocks {layers} are not numbered 0 .. {num_layers - 1}")
        if num_layers == 0 or "backbone.convnext.0.pwconv1.weight" not in own:
            raise ValueError("missing keys: backbone.convnext.0.pwconv1.weight")
        inter = int(own["backbone.convnext.0.pwconv1.weight"].shape[0])
        gamma = "backbone.convnext.0.gamma" in own
        if "head.out.weight" not in own:
            raise ValueError("missing keys: head.out.weight")
        n_fft = int(own["head.out.weight"].shape[0]) - 2
        window = own.get("head.istft.window")
        _check_dims(n_mels, dim, inter, n_fft, int(window.numel()) if window is not None else n_fft, hop_length, padding)
        expected = _official_keys(num_layers, gamma)
        missing = [k for k in expected if k not in own]
        if missing:
            raise ValueError(f"missing keys: {missing[:8]}{' ...' if len(missing) > 8 else ''}")
        model = cls(n_mels, dim, inter, num_layers, gamma, hop_length, padding)
        model.load_state_dict({k: own[k].detach().to(torch.float32) for k in expected}, strict=True)
        return model

    @classmethod
    def from_pretrained(cls, path, hop_length: int = HOP, padding: str = "same") -> "Vocoder":
        """A torch.save'd state dict, a dict holding one under "state_dict", or a TorchScript archive (the notebook's
        vocos_ms_fp16.pts: its parameters and buffers)."""
        with open(path, "rb") as f:
            data = f.read()
        try:
            sd = torch.jit.load(io.BytesIO(data), map_location="cpu").state_dict()
        except RuntimeError:
            obj = torch.load(io.BytesIO(data), map_location="cpu", weights_only=True)
            sd = obj["state_dict"] if isinstance(obj, dict) and "state_dict" in obj else obj
        if not isinstance(sd, dict):
            raise ValueError(f"{os.fspath(path)}: not a state dict, a {{'state_dict': ...}} dict or a TorchScript archive")
        return cls.from_state_dict(sd, hop_length, padding)

    # ---- kernel-ready weight images
    def tables(self) -> Tensor:
        """fp32 [5120]: float64-made twiddles W_2048^m (re, im), then head.istft.window (ispk_istft_head_f32)."""
        w = self.head.istft.window.detach().float()
        return torch.cat([twiddles().to(w.device).flatten(), w]).contiguous()

    def _build(self, dtype: torch.dtype) -> dict:
        bb, cd = self.backbone, dtype
        C, D = self.n_mels, self.dim
        with torch.no_grad():
            emb = bb.embed.weight.detach().float().permute(0, 2, 1).reshape(D, 7 * C)       # column j*C + c: tap j, channel c
            emb_w = torch.zeros((D, self.k_pad), dtype=torch.float32, device=emb.device)
            emb_w[:, :7 * C] = emb
            blocks = []
            for blk in bb.convnext:
                w2, b2 = blk.pwconv2.weight.detach().float(), blk.pwconv2.bias.detach().float()
                if blk.gamma is not None:     # x = gamma * (W2 h + b2)  ->  W2' = diag(gamma) W2, b2' = gamma b2, in fp32
                    g = blk.gamma.detach().float()
                    w2, b2 = w2 * g[:, None], b2 * g
                blocks.append({"dw_w": blk.dwconv.weight.detach().float().reshape(D, 7).contiguous(),
                               "dw_b": blk.dwconv.bias.detach().float().contiguous(),
                               "ln_w": blk.norm.weight.detach().float().contiguous(),
                               "ln_b": blk.norm.bias.detach().float().contiguous(),
                               "w1": blk.pwconv1.weight.detach().to(cd).contiguous(),
                               "b1": blk.pwconv1.bias.detach().float().contiguous(),
                               "w2": w2.to(cd).contiguous(), "b2": b2.contiguous()})
            head_w = torch.zeros((_HEAD_N, D), dtype=torch.float32, device=emb.device)
            head_w[:N_FFT + 2] = self.head.out.weight.detach().float()
            head_b = torch.zeros((_HEAD_N,), dtype=torch.float32, device=emb.device)
            head_b[:N_FFT + 2] = self.head.out.bias.detach().float()
            return {"emb_w": emb_w.to(cd).contiguous(), "emb_b": bb.embed.bias.detach().float().contiguous(),
                    "blocks": blocks, "head_w": head_w.to(cd).contiguous(), "head_b": head_b, "tables": self.tables()}

    # ---- forward
    def _vocode(self, mel: Tensor, mel_len: Optional[Tensor], audio: Tensor, audio_len: Tensor) -> None:
        (B, _, T), cd, dev = mel.shape, self.compute_dtype, mel.device
        R = B * T
        w = self.staged(cd)
        bb = self.backbone
        rows = torch.empty((R, self.k_pad), dtype=cd, device=dev)
        mask = torch.empty((R,), dtype=torch.bool, device=dev)
        runtime.vocoder_unfold(mel, mel_len, rows, mask)
        e = runtime.gemm(rows, w["emb_w"], bias=w["emb_b"], out_dtype=torch.float32)
        x = runtime.layernorm(e, bb.norm.weight, bb.norm.bias, row_mask=mask, eps=EPS)
        x_next = e                                            # the embedding rows are dead: the first block writes there
        for blk in w["blocks"]:
            y = runtime.dwconv7_ln(x, T, blk["dw_w"], blk["dw_b"], blk["ln_w"], blk["ln_b"], mel_len, EPS, out_dtype=cd)
            hid = runtime.gemm(y, blk["w1"], bias=blk["b1"], flags=runtime.EP_GELU, out_dtype=cd)
            runtime.gemm(hid, blk["w2"], bias=blk["b2"], resid=x, mask=mask, flags=runtime.EP_MASK_OUT, out=x_next,
                         out_dtype=torch.float32)
            x, x_next = x_next, x
        y = runtime.layernorm(x, bb.final_layer_norm.weight, bb.final_layer_norm.bias, row_mask=mask, eps=EPS, out_dtype=cd)
        h = runtime.gemm(y, w["head_w"], bias=w["head_b"], out_dtype=torch.float32)
        runtime.istft_head(h, T, mel_len, w["tables"], audio, audio_len)
