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

Launches per call (csrc/hifigan.hip unless noted; the loop is generator.ConvStackGenerator's): ispk_vocoder_unfold + one GEMM
(conv_pre), per stage one ispk_hifigan_upsample and one ispk_hifigan_conv per convolution (leaky-ReLU fused on load, bias /
residual fused on store; the last convolution of each ResBlock adds itself times 1 / J into the stage's sum, so the mean needs
no launch), then ispk_hifigan_post_f32.  V1: 2 + 4 + 72 + 1 = 79 launches; V3: 2 + 3 + 18 + 1 = 24.  No ATen compute op, no host
read: with `out=` buffers a call is capturable.

Batches: utterance b is vocoded as if mel[b, :, :mel_len[b]] were run alone, bit for bit (a workgroup never spans two
utterances and every sum runs in an order fixed by the position inside the utterance); audio_len = hop_length mel_len, samples
past it are 0, nothing past mel_len is read.

Channel counts are multiples of 32 up to 512 (V1, V3).  V2 ends at 16 and 8 channels: NotImplementedError.
"""
from __future__ import annotations

from typing import Sequence

from torch import nn

from . import runtime
from .generator import ConvStackGenerator

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


class HifiGan(ConvStackGenerator):
    """The HiFi-GAN generator on libispk kernels.  Parameters carry the official state-dict names (conv_pre, ups.{i},
    resblocks.{n}.convs1 / convs2 / convs.{m}, conv_post) with plain weight / bias, so a weight-norm-free official dict loads
    with load_state_dict(strict=True); from_state_dict / from_pretrained fold weight norm.  Without a config, blocks of type
    "2" get the V3 table of dilations.  In bf16 compute the output layer stays fp32.

    vocoder = HifiGan.from_pretrained("generator_v1", "config.json").to("cuda").eval()
    audio, audio_len = vocoder(mel, mel_len)        # mel fp32 / fp16 [B, n_mels, T] (any strides), mel_len int64 [B] or None
    audio = vocoder.infer(mel)                      # audio fp32 [B, hop_length T]
    """

    TYPE2_DILATIONS = V3_DILATIONS
    SLOPE = LRELU_SLOPE
    CONV_READS_STAGE = True

    def __init__(self, n_mels: int = 80, upsample_initial_channel: int = 512, upsample_rates: Sequence[int] = (8, 8, 2, 2),
                 upsample_kernel_sizes: Sequence[int] = (16, 16, 4, 4), resblock: str = "1",
                 resblock_kernel_sizes: Sequence[int] = (3, 7, 11),
                 resblock_dilation_sizes: Sequence[Sequence[int]] = ((1, 3, 5),) * 3):
        super().__init__(n_mels, upsample_initial_channel, upsample_rates, upsample_kernel_sizes, resblock,
                         resblock_kernel_sizes, resblock_dilation_sizes)
        C_last = self._stack(_ResBlock1 if self.resblock == "1" else _ResBlock2)
        self.conv_post = nn.Conv1d(C_last, 1, 7, padding=3)

    def _conv_input(self, src, Tl, staged, scratch, kw):
        return (src, *staged)                   # the convolution reads the stage tensor; its leaky-ReLU is fused on load

    def _post(self, x, Tl, w, scratch, audio, audio_len, kw):
        runtime.hifigan_post(x, Tl, w["post_w"], w["post_b"], audio, audio_len, slope=POST_SLOPE, **kw)
