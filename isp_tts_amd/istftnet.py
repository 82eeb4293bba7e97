"""iSTFTNet generator (Kaneko et al., ICASSP 2022; the public `C8C8I` checkpoints and any geometry of the family): mel
spectrograms [B, n_mels, T] -> waveforms.  HiFi-GAN's first stages, then a small inverse STFT in place of the last ones.  The
mel is HiFi-GAN's (22,050 Hz, n_fft 1024, hop 256, 80 slaney mels), the one `data.AcousticFeatures` extracts and the acoustic
model predicts.  Same call surface as `hifigan.HifiGan`: vocoder(mel, mel_len) -> (audio, audio_len).

    x = conv_pre(mel)                                                    Conv1d(n_mels, C0, 7, padding 3)
    for stage i:  x = ups[i](leaky_relu(x, 0.1));  x = mean_j resblocks[i J + j](x)          (HiFi-GAN's, unchanged)
    x = leaky_relu(x, 0.01)
    x = ReflectionPad1d((1, 0))(x)                   one frame in front: p[0] = x[1], p[i] = x[i - 1];  F = R + 1 frames
    y = conv_post(x)                                 Conv1d(C_last, n_fft + 2, 7, padding 3) on the PADDED sequence
    mag   = exp(y[:, :n_fft / 2 + 1])
    phase = phase_scale * sin(y[:, n_fft / 2 + 1:])                      official: phase_scale 1 (sin's value IS the angle)
    audio = torch.istft(mag * exp(1j * phase), n_fft, hop, n_fft, hann_window(n_fft, periodic=True), center=True)

R is the number of rows after the last stage; the output has hop (F - 1) = hop R samples per utterance, so hop_length =
prod(upsample_rates) * hop: 8 * 8 * 4 = 256 for C8C8I.  irfft ignores the imaginary parts of the DC and Nyquist bins; the
envelope sum_f w^2 runs over the frames of the utterance, so it leaves its interior value 1.5 in the first and last n_fft / 2
samples of EACH utterance, not of the padded batch.

Launches per call: ispk_vocoder_unfold + one GEMM (conv_pre), per stage one ispk_hifigan_upsample and one ispk_hifigan_conv
per convolution (generator.ConvStackGenerator's loop on csrc/hifigan.hip), then ONE ispk_istftnet_head_f32 (csrc/istftnet.hip)
for everything from the last leaky-ReLU to the waveform.  C8C8I: 2 + 2 + 36 + 1 = 41 launches (HiFi-GAN V1: 79), and no tensor
longer than 64 rows per mel frame.  No ATen compute op, no host read: with `out=` buffers a call is capturable.

Batches: as HifiGan - utterance b is vocoded as if mel[b, :, :mel_len[b]] were run alone, bit for bit; audio_len = hop_length
mel_len, samples past it are 0, nothing past mel_len is read.  An utterance needs R >= 2 rows for the reflection: the product
of the upsampling rates is at least 2 (NotImplementedError otherwise), so every mel_len >= 1 has them.

n_fft is a multiple of 4 from 8 to 32 with hop = n_fft / 4 (the official geometry is 16 / 4).  In bf16 compute the output
layer stays fp32.
"""
from __future__ import annotations

import math
from typing import Sequence

from torch import nn

from . import runtime
from .generator import ConvStackGenerator
from .hifigan import LRELU_SLOPE, POST_SLOPE, V3_DILATIONS, _ResBlock1, _ResBlock2

CONFIGS = {
    "c8c8i": dict(n_mels=80, upsample_initial_channel=512, upsample_rates=(8, 8), upsample_kernel_sizes=(16, 16),
                  resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3,
                  gen_istft_n_fft=16, gen_istft_hop_size=4),
}


class IstftNet(ConvStackGenerator):
    """The iSTFTNet generator on libispk kernels.  Parameters carry the official state-dict names (HiFi-GAN's: conv_pre,
    ups.{i}, resblocks.{n}.convs1 / convs2 / convs.{m}, conv_post) with plain weight / bias; from_state_dict / from_pretrained
    fold weight norm, read n_fft from conv_post's shape and the hop from the config's gen_istft_hop_size (default n_fft / 4).

    vocoder = IstftNet.from_pretrained("g_00975000", "config.json").to("cuda").eval()
    audio, audio_len = vocoder(mel, mel_len)        # mel fp32 / fp16 [B, n_mels, T] (any strides), mel_len int64 [B] or None
    audio = vocoder.infer(mel)                      # audio fp32 [B, hop_length T]
    """

    TYPE2_DILATIONS = V3_DILATIONS
    SLOPE = LRELU_SLOPE
    CONV_READS_STAGE = True

    def __init__(self, n_mels: int = 80, upsample_initial_channel: int = 512, upsample_rates: Sequence[int] = (8, 8),
                 upsample_kernel_sizes: Sequence[int] = (16, 16), resblock: str = "1",
                 resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                 resblock_dilation_sizes: Sequence[Sequence[int]] = ((1, 3, 5),) * 3, gen_istft_n_fft: int = 16,
                 gen_istft_hop_size: int = 4, phase_scale: float = 1.0):
        n_fft, hop = int(gen_istft_n_fft), int(gen_istft_hop_size)
        if n_fft not in runtime.ISTFTNET_N_FFTS:
            raise NotImplementedError(f"gen_istft_n_fft {n_fft}: {runtime.ISTFTNET_N_FFTS} are built")
        if hop * 4 != n_fft:
            raise NotImplementedError(f"gen_istft_hop_size {hop} with gen_istft_n_fft {n_fft}: hop = n_fft / 4 is built")
        if math.prod(int(u) for u in upsample_rates) < 2:
            raise NotImplementedError(f"upsample_rates {tuple(upsample_rates)}: the reflection pad needs two rows per mel frame, "
                                      f"a product of at least 2 is built")
        super().__init__(n_mels, upsample_initial_channel, upsample_rates, upsample_kernel_sizes, resblock,
                         resblock_kernel_sizes, resblock_dilation_sizes, head_hop=hop)
        self.n_fft, self.istft_hop, self.phase_scale = n_fft, hop, float(phase_scale)
        C_last = self._stack(_ResBlock1 if self.resblock == "1" else _ResBlock2)
        self.conv_post = nn.Conv1d(C_last, n_fft + 2, 7, padding=3)

    def config(self) -> dict:
        return dict(super().config(), gen_istft_n_fft=self.n_fft, gen_istft_hop_size=self.istft_hop,
                    phase_scale=self.phase_scale)

    @classmethod
    def _extra_args(cls, own: dict, cfg: dict) -> tuple:
        if "conv_post.weight" not in own:
            raise ValueError("missing keys: conv_post.weight")
        n_fft = int(own["conv_post.weight"].shape[0]) - 2
        if "gen_istft_n_fft" in cfg and int(cfg["gen_istft_n_fft"]) != n_fft:
            raise ValueError(f"config does not fit the weights: gen_istft_n_fft {cfg['gen_istft_n_fft']}, conv_post has "
                             f"{n_fft + 2} = n_fft + 2 output channels")
        return n_fft, int(cfg.get("gen_istft_hop_size", n_fft // 4)), float(cfg.get("phase_scale", 1.0))

    def _build(self, dtype) -> dict:
        w = super()._build(dtype)
        # [n_fft + 2, C, 7] -> [7, n_fft + 2, C], fp32 in either compute dtype; the twiddles and the window from float64
        w["post_w"] = self.conv_post.weight.detach().float().permute(2, 0, 1).contiguous()
        w["post_table"] = runtime.istftnet_table(self.n_fft).to(w["post_w"].device)
        return w

    def _conv_input(self, src, Tl, staged, scratch, kw):
        return (src, *staged)                   # the convolution reads the stage tensor; its leaky-ReLU is fused on load

    def _post(self, x, Tl, w, scratch, audio, audio_len, kw):
        runtime.istftnet_head(x, Tl, w["post_w"], w["post_b"], w["post_table"], self.n_fft, self.istft_hop, audio, audio_len,
                              slope=POST_SLOPE, phase_scale=self.phase_scale, **kw)
