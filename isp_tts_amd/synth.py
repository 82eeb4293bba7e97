"""Deterministic synthetic weights and inputs.

There is no network on the build or GPU boxes, so checkpoints are unavailable;
every test, golden fixture and benchmark uses weights produced here.  Each tensor is drawn from
its own counter-based stream keyed by the parameter NAME, so the values are identical in this
container, on the GPU box and inside the golden-fixture generator without committing any weights.

The parameter names/shapes are the reference's `state_dict` layout (verified against the
reference's own key list in tests/golden/state_dict_keys.json).
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch

from .config import AcousticDims
from .hifigan import CONFIGS as _HIFIGAN_CONFIGS
from .istftnet import CONFIGS as _ISTFTNET_CONFIGS

SEED = 23  # recipe seed (recipes/acoustic/core.yaml:5)


def _rng(name: str, seed: int = SEED) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[zlib.crc32(name.encode()), seed]))


def _normal(name: str, shape, scale: float = 1.0, shift: float = 0.0, seed: int = SEED) -> torch.Tensor:
    x = _rng(name, seed).standard_normal(size=tuple(shape)) * scale + shift
    return torch.from_numpy(x.astype(np.float32))


def alibi_default_slopes(heads: int) -> list[float]:
    """ALiBi geometric slopes (embeddings.py:38-49 of the reference): for a power-of-two head count
    2^(-8/n * (i+1)); otherwise the closest lower power of two plus every other slope of the next one."""
    def pow2(n):
        start = 2.0 ** (-(2.0 ** -(math.log2(n) - 3)))
        return [start * start ** i for i in range(n)]
    if math.log2(heads).is_integer():
        return pow2(heads)
    n = 2 ** math.floor(math.log2(heads))
    return pow2(n) + pow2(2 * n)[0::2][: heads - n]


def _transformer_spec(prefix: str, dim: int, depth: int, heads: int, ffn: int, emb_dim: int,
                      adaptive: bool, cond_dim: int) -> list[tuple]:
    spec = []
    for i in range(depth):
        p = f"{prefix}.layers.{i}"
        for norm in ("attention_norm", "feed_forward_norm"):
            if adaptive:
                spec += [(f"{p}.{norm}.weight.weight", (dim, cond_dim), "ada_w"),
                         (f"{p}.{norm}.weight.bias", (dim,), "gamma"),
                         (f"{p}.{norm}.bias.weight", (dim, cond_dim), "ada_w"),
                         (f"{p}.{norm}.bias.bias", (dim,), "beta")]
            else:
                spec += [(f"{p}.{norm}.weight", (dim,), "gamma"), (f"{p}.{norm}.bias", (dim,), "beta")]
            if norm == "attention_norm":
                spec += [(f"{p}.attention.to_q.weight", (heads * 64, dim), "linear"),
                         (f"{p}.attention.to_kv.weight", (128, dim), "linear"),
                         (f"{p}.attention.rel_pos.learned_logslopes", (heads, 1, 1), "logslopes"),
                         (f"{p}.attention.to_out.weight", (dim, heads * 64), "linear")]
        spec += [(f"{p}.feed_forward.net.0.weight", (ffn, dim), "linear"),
                 (f"{p}.feed_forward.net.3.weight", (dim, ffn), "linear")]
    if emb_dim != dim:
        spec += [(f"{prefix}.project_emb.weight", (dim, emb_dim), "linear"),
                 (f"{prefix}.project_emb.bias", (dim,), "beta")]
    spec += [(f"{prefix}.norm.weight", (dim,), "gamma"), (f"{prefix}.norm.bias", (dim,), "beta")]
    return spec


def model_spec(dims: AcousticDims = AcousticDims()) -> list[tuple]:
    """(name, shape, kind) for every entry of the reference state_dict, in its order."""
    d, a = dims.text_dim, dims.ada_dim
    spec = [("pitch_mean", (), "zero"), ("pitch_std", (), "one"),
            ("text_embedding.weight", (dims.vocab, d), "embedding")]
    spec += _transformer_spec("encoder", d, dims.enc_depth, dims.heads, dims.ffn, d, False, 0)
    kk, (q0, q1) = dims.key_kernel, dims.query_kernels
    al = "aligner.attention"
    spec += [(f"{al}.key_proj.0.conv.weight", (2 * d, d, kk), "conv"),
             (f"{al}.key_proj.0.norm.weight", (2 * d,), "gamma"), (f"{al}.key_proj.0.norm.bias", (2 * d,), "beta"),
             (f"{al}.key_proj.1.conv.weight", (dims.attn_dim, 2 * d, 1), "conv"),
             (f"{al}.query_proj.0.conv.weight", (2 * dims.mel_dim, dims.mel_dim, q0), "conv"),
             (f"{al}.query_proj.0.norm.weight", (2 * dims.mel_dim,), "gamma"),
             (f"{al}.query_proj.0.norm.bias", (2 * dims.mel_dim,), "beta"),
             (f"{al}.query_proj.1.conv.weight", (dims.mel_dim, 2 * dims.mel_dim, q1), "conv"),
             (f"{al}.query_proj.1.norm.weight", (dims.mel_dim,), "gamma"),
             (f"{al}.query_proj.1.norm.bias", (dims.mel_dim,), "beta"),
             (f"{al}.query_proj.2.conv.weight", (dims.attn_dim, dims.mel_dim, 1), "conv")]
    tp = "temporal_adaptor.predictor"
    spec += [(f"{tp}.time_embedding.freq_emb.freq_scale", (1,), "freq_scale"),
             (f"{tp}.time_embedding.mlp.0.weight", (dims.time_dim, 65), "linear"),
             (f"{tp}.time_embedding.mlp.0.bias", (dims.time_dim,), "beta"),
             (f"{tp}.time_embedding.mlp.2.weight", (dims.time_dim, dims.time_dim), "linear"),
             (f"{tp}.time_embedding.mlp.2.bias", (dims.time_dim,), "beta")]
    spec += _transformer_spec(f"{tp}.transformer", a, dims.ada_depth, dims.ada_heads, dims.ada_ffn, d + 3, True,
                              dims.time_dim)
    spec += [(f"{tp}.linear_layer.weight", (3, a), "linear"), (f"{tp}.linear_layer.bias", (3,), "beta")]
    te = "temporal_adaptor.embedding"
    spec += _transformer_spec(f"{te}.transformer", a, dims.emb_depth, dims.ada_heads, dims.ada_ffn, 2, False, 0)
    spec += [(f"{te}.linear_layer.weight", (d, a), "linear"), (f"{te}.linear_layer.bias", (d,), "beta")]
    spec += _transformer_spec("decoder", d, dims.dec_depth, dims.heads, dims.ffn, d, False, 0)
    spec += [("to_mel.weight", (dims.mel_dim, d), "linear"), ("to_mel.bias", (dims.mel_dim,), "beta")]
    return spec


def make_state_dict(dims: AcousticDims = AcousticDims(), seed: int = SEED) -> dict[str, torch.Tensor]:
    """fp32 CPU tensors for every state_dict entry.  Scales are chosen so activations stay O(1) through
    the 12 pre-norm layers (so that an absolute 1e-4 mel tolerance is a meaningful bar)."""
    sd = {}
    for name, shape, kind in model_spec(dims):
        if kind == "zero":
            t = torch.tensor(0.0)
        elif kind == "one":
            t = torch.tensor(1.0)
        elif kind == "freq_scale":
            t = torch.full((1,), 1000.0)
        elif kind == "embedding":
            t = _normal(name, shape, seed=seed)
            t[0].zero_()  # padding_idx = 0
        elif kind == "linear":
            t = _normal(name, shape, 1.0 / math.sqrt(shape[1]), seed=seed)
        elif kind == "conv":
            t = _normal(name, shape, 1.0 / math.sqrt(shape[1] * shape[2]), seed=seed)
        elif kind == "gamma":
            t = _normal(name, shape, 0.1, 1.0, seed=seed)
        elif kind == "beta":
            t = _normal(name, shape, 0.1, seed=seed)
        elif kind == "ada_w":
            t = _normal(name, shape, 0.1 / math.sqrt(shape[1]), seed=seed)
        elif kind == "logslopes":
            # float64 libm then one rounding: identical on every host (fp32 vector log is not)
            base = torch.tensor([math.log(v) for v in alibi_default_slopes(shape[0])], dtype=torch.float64)
            t = (base.view(shape) + _normal(name, shape, 0.1, seed=seed).double()).float()
        else:
            raise KeyError(kind)
        sd[name] = t.contiguous()
    return sd


def make_speaker_table(num_speakers: int, dims: AcousticDims = AcousticDims(), seed: int = SEED) -> torch.Tensor:
    """`speaker_embedding.weight` [num_speakers, encoder dim] of a multi-speaker model (model.py:93-97), O(0.3) entries so that
    the speaker shift is visible against the O(1) encoder output."""
    return _normal("speaker_embedding.weight", (num_speakers, dims.text_dim), 0.3, seed=seed).contiguous()


def make_lengths(batch: int, text_max: int, mel_max: int, variable: bool, seed: int = SEED):
    """Fixed-length batches (BASELINE configs 2-3) or the variable-length rule of config 4:
    mel_len ~ U{mel_max/8 .. mel_max}, text_len = clamp(round(mel_len / 5.12), 25, text_max) <= mel_len.
    Item 0 always has the maximum lengths so the padded shapes are (text_max, mel_max)."""
    if not variable:
        return (torch.full((batch,), text_max, dtype=torch.int64), torch.full((batch,), mel_max, dtype=torch.int64))
    g = _rng(f"lengths/{batch}/{text_max}/{mel_max}", seed)
    mel_len = g.integers(max(mel_max // 8, 4), mel_max + 1, size=batch)
    mel_len[0] = mel_max
    lo = min(25, text_max)
    text_len = np.clip(np.rint(mel_len / (mel_max / text_max)).astype(np.int64), lo, text_max)
    text_len = np.minimum(text_len, mel_len)
    text_len[0] = text_max
    return torch.from_numpy(text_len.astype(np.int64)), torch.from_numpy(mel_len.astype(np.int64))


def make_inputs(batch: int, text_max: int = 100, mel_max: int = 512, variable: bool = False,
                dims: AcousticDims = AcousticDims(), seed: int = SEED) -> dict[str, torch.Tensor]:
    """Synthetic random-phoneme batch in the collator's layout (collator.py:36-55 of the reference):
    text int64 [B,L] zero-padded, mel fp32 [B,80,M], pitch/energy fp32 [B,M], lengths int64 [B]."""
    tag = f"inputs/{batch}/{text_max}/{mel_max}/{int(variable)}"
    g = _rng(tag, seed)
    text_len, mel_len = make_lengths(batch, text_max, mel_max, variable, seed)
    text = torch.from_numpy(g.integers(2, dims.vocab, size=(batch, text_max)).astype(np.int64))
    mel = torch.from_numpy((g.standard_normal((batch, dims.mel_dim, mel_max)) * 2.0 - 5.0).astype(np.float32))
    mel = mel.clamp_(min=math.log(1e-5))
    pitch = torch.from_numpy(g.standard_normal((batch, mel_max)).astype(np.float32))
    # float64 log1p rounded once to fp32 (host-independent, unlike torch's vectorised fp32 log1p)
    energy = torch.from_numpy(np.log1p(np.abs(g.standard_normal((batch, mel_max))) * 5.0).astype(np.float32))
    tmask = torch.arange(text_max)[None] < text_len[:, None]
    mmask = torch.arange(mel_max)[None] < mel_len[:, None]
    text = text * tmask
    mel = mel * mmask[:, None]
    pitch = pitch * mmask
    energy = energy * mmask
    # flow-matching noise is an INPUT here (generated on the host, SURVEY 7 "Randomness"):
    x0 = torch.from_numpy(g.standard_normal((batch, text_max, 3)).astype(np.float32))
    t = torch.from_numpy(g.random(batch).astype(np.float32))
    return {"text": text, "text_len": text_len, "mel": mel, "mel_len": mel_len, "pitch": pitch, "energy": energy,
            "flow_x0": x0, "flow_t": t}


def make_mas_logits(batch: int, mel_max: int, text_max: int, variable: bool = False, kind: str = "realistic",
                    seed: int = SEED):
    """Aligner-like MAS inputs, built from IEEE-exact operations only (+, -, *, /, max) so that every host produces
    the same bits: "realistic" = N(0,1) noise plus the log of the reference's diagonal prior
    (-(t/T - m/M)^2 / (2 * 0.1^2), floored at log(1e-6) like `log(prior + 1e-6)`, alignment.py:196; per-row
    normalisation constants are dropped because MAS is invariant to them); "ties" = small integers, which force the
    tie-breaking rule (ties -> diagonal, mas.py:17 of the reference)."""
    g = _rng(f"mas/{batch}/{mel_max}/{text_max}/{int(variable)}/{kind}", seed)
    text_len, mel_len = make_lengths(batch, text_max, mel_max, variable, seed)
    if kind == "ties":
        x = torch.from_numpy(g.integers(-3, 1, size=(batch, mel_max, text_max)).astype(np.float32))
    else:
        z = torch.from_numpy(g.standard_normal((batch, mel_max, text_max)).astype(np.float32))
        ti = torch.arange(text_max, dtype=torch.float32)[None, None, :] / text_len[:, None, None].float()
        mi = torch.arange(mel_max, dtype=torch.float32)[None, :, None] / mel_len[:, None, None].float()
        d = ti - mi
        x = z + torch.clamp(-(d * d) * 50.0, min=-13.815511)
    return x.contiguous(), text_len, mel_len


# (B, T, L, mel layout, mel_len, text_len, attention kind) of the evaluator fixture's synthetic cases (tests/golden/metrics.npz)
METRIC_CASES = {
    "ragged": (5, 77, 23, "bct", [77, 1, 40, 76, 33], [23, 1, 9, 1, 12], "soft"),
    "ties": (3, 70, 9, "bct", [70, 64, 33], [9, 5, 7], "ties"),
    "t80": (2, 80, 17, "btc", [80, 41], [17, 6], "soft"),        # [B, 80, 80]: the reference reads it frames-first
    "btc": (3, 100, 31, "btc", [100, 57, 2], [31, 20, 2], "soft"),
}


def make_metric_inputs(case: str, seed: int = SEED) -> dict[str, torch.Tensor]:
    """Inputs of one evaluator case (models/acoustic/evaluator.py), from IEEE-exact operations on a keyed stream:
    mel_out / mel_target fp32 [B, 80, T] ("bct") or [B, T, 80] ("btc"); the target is zero past mel_len (the collator's
    padding), the prediction is not (MCD counts every frame).  attn_soft fp32 [B, T, L]: normalised squares of uniform draws
    ("soft") or small multiples of 1/4 with many exact row ties ("ties"), non-zero on padded frames too (the strength sums
    every frame).  max(mel_len) == T, as the reference's boolean mask requires."""
    B, T, L, layout, mel_len, text_len, kind = METRIC_CASES[case]
    g = _rng(f"metrics/{case}", seed)
    target = g.standard_normal((B, 80, T)) * 2.0 - 5.0
    out = target + g.standard_normal((B, 80, T)) * 0.5
    target = target * (np.arange(T)[None, None, :] < np.asarray(mel_len)[:, None, None])
    if kind == "ties":
        attn = g.integers(0, 4, size=(B, T, L)) * 0.25
    else:
        r = g.random((B, T, L))
        attn = r * r
        attn = attn / attn.sum(axis=-1, keepdims=True)
    if layout == "btc":
        out, target = out.transpose(0, 2, 1), target.transpose(0, 2, 1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))   # noqa: E731
    return {"mel_out": f32(out), "mel_target": f32(target), "attn_soft": f32(attn),
            "mel_len": torch.tensor(mel_len, dtype=torch.int64), "text_len": torch.tensor(text_len, dtype=torch.int64)}


# (kind, samples, peak amplitude) of the feature extractor's test clips; FEATURE_CASES name the fixture's batches
# (tests/golden/features.npz).  Lengths cover one frame (256), the YIN pad edge (281 / 282 / 283) and the pitch-count
# quirk (k 256 + 25 / 26 / 27).
CLIP_KINDS = ("harmonic", "noise", "silence", "edge_hi", "edge_lo", "chirp")
FEATURE_CASES = {
    "edges": [("harmonic", 256, 0.5), ("noise", 257, 0.3), ("edge_hi", 281, 0.9), ("harmonic", 282, 1.0),
              ("chirp", 283, 0.5), ("edge_lo", 2 * 256 + 25, 0.5), ("harmonic", 3 * 256 + 26, 0.2),
              ("noise", 4 * 256 + 27, 0.5), ("harmonic", 5 * 256, 0.7)],
    "voices": [("harmonic", 11025, 0.8), ("chirp", 12000, 0.6), ("edge_hi", 6400 + 26, 1.0), ("edge_lo", 9000, 0.9),
               ("noise", 7000, 0.5), ("silence", 5000, 0.0), ("harmonic", 8192, 1e-4), ("chirp", 10000 + 25, 1e-2)],
}


def make_clip(kind: str, samples: int, amplitude: float = 0.5, seed: int = SEED, sample_rate: int = 22050) -> torch.Tensor:
    """A deterministic fp32 test waveform from a keyed stream, peak |x| = amplitude: "harmonic" (six partials of a 90-300 Hz
    f0 with 5.5 Hz vibrato, plus a little noise), "noise", "silence", "edge_hi" (a 700 -> 800 Hz glide up to torch-yin's upper
    search edge) / "edge_lo" (a tone at its 42 Hz lower edge), "chirp" (a 100 -> 400 Hz sweep gated on and off every 0.1 s, noise in the gaps)."""
    if kind not in CLIP_KINDS:
        raise ValueError(f"unknown clip kind {kind!r}")
    g = _rng(f"clip/{kind}/{samples}/{amplitude!r}", seed)
    t = np.arange(samples, dtype=np.float64) / sample_rate
    if kind == "harmonic":
        f0 = g.uniform(90.0, 300.0) * (1.0 + 0.03 * np.sin(2 * np.pi * 5.5 * t + g.uniform(0, 2 * np.pi)))
        ph = 2 * np.pi * np.cumsum(f0) / sample_rate
        x = sum(0.7 ** h * np.sin(h * ph + g.uniform(0, 2 * np.pi)) for h in range(1, 7)) + 0.01 * g.standard_normal(samples)
    elif kind == "noise":
        x = g.standard_normal(samples)
    elif kind == "silence":
        x = np.zeros(samples)
    elif kind == "edge_hi":         # 700 -> 800 Hz: periods from 31.5 down to the 27.6 samples of torch-yin's upper edge
        x = np.sin(2 * np.pi * np.cumsum(700.0 + 100.0 * t / max(t[-1], 1e-9)) / sample_rate + g.uniform(0, 2 * np.pi))
    elif kind == "edge_lo":
        x = np.sin(2 * np.pi * 42.0 * t + g.uniform(0, 2 * np.pi)) + 0.3 * np.sin(2 * np.pi * 84.0 * t)
    else:
        f = 100.0 * 4.0 ** (t / max(t[-1], 1e-9)) if samples > 1 else np.full(samples, 100.0)
        voiced = (np.floor(t / 0.1) % 2) == 0
        x = np.where(voiced, np.sin(2 * np.pi * np.cumsum(f) / sample_rate), 0.3 * g.standard_normal(samples))
    peak = np.abs(x).max() if samples else 0.0
    x = x * (amplitude / peak) if peak > 0 else x
    return torch.from_numpy(x.astype(np.float32))


def make_feature_case(case: str, seed: int = SEED) -> list[torch.Tensor]:
    return [make_clip(k, n, a, seed) for k, n, a in FEATURE_CASES[case]]


VOCODER_DIMS = {"official": (80, 512, 1536, 8), "small": (100, 384, 1152, 3)}   # (n_mels, dim, intermediate, layers)


def make_vocoder_state_dict(dims=VOCODER_DIMS["official"], seed: int = SEED, gamma: bool = True) -> dict[str, torch.Tensor]:
    """Synthetic Vocos (mel variant) weights in the official state-dict layout (backbone.*, head.*), from keyed streams.
    dims = (n_mels, dim, intermediate, layers).  The head is scaled so that, on LayerNorm-ed rows, the log-magnitude
    (N(0.5, 2.5^2)-like) lies on both sides of the log(100) clip and the phase carries a per-bin offset of up to +-300 rad
    (sincos far outside [-pi, pi]) plus an N(0, 2^2) data-dependent part."""
    n_mels, dim, inter, layers = dims
    u = lambda name, shape, lo, hi: torch.from_numpy(_rng(name, seed).uniform(lo, hi, size=tuple(shape)).astype(np.float32))
    sd = {"backbone.embed.weight": _normal("voc/embed.w", (dim, n_mels, 7), 1.0 / math.sqrt(7 * n_mels), seed=seed),
          "backbone.embed.bias": _normal("voc/embed.b", (dim,), 0.1, seed=seed),
          "backbone.norm.weight": _normal("voc/norm.w", (dim,), 0.1, 1.0, seed=seed),
          "backbone.norm.bias": _normal("voc/norm.b", (dim,), 0.1, seed=seed)}
    for i in range(layers):
        p = f"backbone.convnext.{i}."
        sd[p + "dwconv.weight"] = _normal(f"voc/{i}/dw.w", (dim, 1, 7), 1.0 / math.sqrt(7), seed=seed)
        sd[p + "dwconv.bias"] = _normal(f"voc/{i}/dw.b", (dim,), 0.1, seed=seed)
        sd[p + "norm.weight"] = _normal(f"voc/{i}/ln.w", (dim,), 0.1, 1.0, seed=seed)
        sd[p + "norm.bias"] = _normal(f"voc/{i}/ln.b", (dim,), 0.1, seed=seed)
        sd[p + "pwconv1.weight"] = _normal(f"voc/{i}/pw1.w", (inter, dim), 1.0 / math.sqrt(dim), seed=seed)
        sd[p + "pwconv1.bias"] = _normal(f"voc/{i}/pw1.b", (inter,), 0.1, seed=seed)
        sd[p + "pwconv2.weight"] = _normal(f"voc/{i}/pw2.w", (dim, inter), 1.0 / math.sqrt(inter), seed=seed)
        sd[p + "pwconv2.bias"] = _normal(f"voc/{i}/pw2.b", (dim,), 0.1, seed=seed)
        if gamma:
            sd[p + "gamma"] = u(f"voc/{i}/gamma", (dim,), 0.05, 0.5)
    sd["backbone.final_layer_norm.weight"] = _normal("voc/fln.w", (dim,), 0.1, 1.0, seed=seed)
    sd["backbone.final_layer_norm.bias"] = _normal("voc/fln.b", (dim,), 0.1, seed=seed)
    sd["head.out.weight"] = torch.cat([_normal("voc/head.mag.w", (513, dim), 2.5 / math.sqrt(dim), seed=seed),
                                       _normal("voc/head.ph.w", (513, dim), 2.0 / math.sqrt(dim), seed=seed)])
    sd["head.out.bias"] = torch.cat([_normal("voc/head.mag.b", (513,), 0.5, 0.5, seed=seed),
                                     u("voc/head.ph.b", (513,), -300.0, 300.0)])
    sd["head.istft.window"] = torch.hann_window(1024)
    return sd


def make_vocoder_mel(B: int, n_mels: int, T: int, seed: int = SEED) -> torch.Tensor:
    """A log-mel-like fp32 [B, n_mels, T] input (smooth in time, values around -11 .. 2)."""
    g = _rng(f"voc/mel/{B}/{n_mels}/{T}", seed)
    x = g.standard_normal((B, n_mels, T + 4)) * 1.5
    x = (x[..., :-4] + x[..., 1:-3] + x[..., 2:-2] + x[..., 3:-1] + x[..., 4:]) / 5 * 2.0
    return torch.from_numpy((x - 4.5 + np.linspace(1.5, -1.5, n_mels)[None, :, None]).astype(np.float32))


# ------------------------------------------------------------------------------------- HiFi-GAN and BigVGAN generators
def _make_generator(tag: str, dims: dict, seed: int, weight_norm: Optional[str], s_pre: float, s_up: float, s_unit: dict,
                    s_post: float, up_key: str = "ups.{i}", act=None, post_bias: bool = True,
                    post_channels: int = 1) -> dict[str, torch.Tensor]:
    """The walk over conv_pre, stages, blocks, units and conv_post that both generator families share, on the streams
    `<tag>/<name>.w|.f|.b`.  Convolution weights are N(0, s^2 / fan_in): s_pre, s_up (fan_in C_in k / stride), s_unit[type] per
    convolution of a unit, s_post; biases N(0, 0.05^2).  `act(sd, name, C)`, if given, adds the activation that precedes each
    unit convolution (after the unit's weights) and activation_post.  conv_post has `post_channels` outputs (1: a waveform).
    weight_norm None: plain `weight`; "g_v": `weight_g` + `weight_v`; "parametrized": `parametrizations.weight.original0` + `original1`.  v is the plain weight times a per-slice
    factor in [0.5, 2] and g the plain weight's norm, so g != ||v|| and g v / ||v|| is the plain weight."""
    if weight_norm not in (None, "g_v", "parametrized"):
        raise ValueError(f"weight_norm {weight_norm!r}: None, 'g_v' or 'parametrized'")
    C0, rates, up_k = dims["upsample_initial_channel"], dims["upsample_rates"], dims["upsample_kernel_sizes"]
    sd: dict[str, torch.Tensor] = {}

    def put(name: str, shape, fan: float, s: float, bias: bool = True):
        w = _normal(f"{tag}/{name}.w", shape, s / math.sqrt(fan), seed=seed)
        if weight_norm is None:
            sd[name + ".weight"] = w
        else:
            gk, vk = (".weight_g", ".weight_v") if weight_norm == "g_v" else (".parametrizations.weight.original0",
                                                                             ".parametrizations.weight.original1")
            ones = [1] * (len(shape) - 1)
            f = torch.from_numpy(_rng(f"{tag}/{name}.f", seed).uniform(0.5, 2.0, size=(shape[0], *ones)).astype(np.float32))
            sd[name + gk] = w.double().flatten(1).norm(dim=1).reshape(shape[0], *ones).float()
            sd[name + vk] = w * f
        if bias:
            sd[name + ".bias"] = _normal(f"{tag}/{name}.b", (shape[0] if not name.startswith("ups.") else shape[1],), 0.05, seed=seed)

    put("conv_pre", (C0, dims["n_mels"], 7), dims["n_mels"] * 7, s_pre)
    J = len(dims["resblock_kernel_sizes"])
    convs = ("convs1", "convs2") if str(dims["resblock"]) == "1" else ("convs",)
    for i, (u, k) in enumerate(zip(rates, up_k)):
        C = C0 >> i
        put(up_key.format(i=i), (C, C // 2, k), C * k / u, s_up)
        for j, (r, D) in enumerate(zip(dims["resblock_kernel_sizes"], dims["resblock_dilation_sizes"])):
            n = i * J + j
            for m in range(len(D)):
                for name, s in zip(convs, s_unit[str(dims["resblock"])]):
                    put(f"resblocks.{n}.{name}.{m}", (C // 2, C // 2, r), C // 2 * r, s)
                if act:
                    for l in range(len(convs) * m, len(convs) * (m + 1)):
                        act(sd, f"resblocks.{n}.activations.{l}", C // 2)
    C = C0 >> len(rates)
    if act:
        act(sd, "activation_post", C)
    put("conv_post", (post_channels, C, 7), C * 7, s_post, bias=post_bias)
    return sd


# name -> generator configuration (hifigan.HifiGan's constructor arguments); "v1" and "v3" are hifigan.CONFIGS' own.  "odd":
# stage lengths that are no powers of two, unequal taps per phase (k 7, stride 3) and the 25-row halo of k 11, dilation 5.
HIFIGAN_DIMS = {
    "v1": _HIFIGAN_CONFIGS["v1"],
    "v3": _HIFIGAN_CONFIGS["v3"],
    "odd": dict(n_mels=20, upsample_initial_channel=128, upsample_rates=(3, 2), upsample_kernel_sizes=(7, 4),
                resblock="1", resblock_kernel_sizes=(3, 11), resblock_dilation_sizes=((1, 3, 5),) * 2),
}


def make_hifigan_state_dict(dims=HIFIGAN_DIMS["v1"], seed: int = SEED, weight_norm: Optional[str] = None) -> dict[str, torch.Tensor]:
    """Synthetic HiFi-GAN generator weights in the official state-dict layout, from keyed streams.  Convolution weights are
    N(0, s^2 / (C_in k)) with s = 1.4 (first convolution of a type "1" unit), 0.5 (second), 0.7 (type "2"), up-convolutions
    N(0, 1.4^2 / (C_in k / stride)), conv_post s = 0.1, biases N(0, 0.05^2): on make_vocoder_mel the output peaks at
    0.16 - 0.9, inside tanh's curved part.  weight_norm: see _make_generator."""
    return _make_generator("hfg", dims, seed, weight_norm, 1.0, 1.4, {"1": (1.4, 0.5), "2": (0.7,)}, 0.1)


# name -> generator configuration (istftnet.IstftNet's constructor arguments).  "c8c8i": istftnet.CONFIGS' own.  "odd":
# HIFIGAN_DIMS["odd"]'s stages (lengths that are no powers of two) under an 8 / 2 inverse STFT.  "n20": blocks of type "2", a
# 20 / 5 inverse STFT (a post layer of 22 channels, twiddles that are no powers of two) and phase_scale = pi.
ISTFTNET_DIMS = {
    "c8c8i": _ISTFTNET_CONFIGS["c8c8i"],
    "odd": dict(n_mels=20, upsample_initial_channel=128, upsample_rates=(3, 2), upsample_kernel_sizes=(7, 4),
                resblock="1", resblock_kernel_sizes=(3, 11), resblock_dilation_sizes=((1, 3, 5),) * 2,
                gen_istft_n_fft=8, gen_istft_hop_size=2),
    "n20": dict(n_mels=20, upsample_initial_channel=128, upsample_rates=(3, 2), upsample_kernel_sizes=(7, 4),
                resblock="2", resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)),
                gen_istft_n_fft=20, gen_istft_hop_size=5, phase_scale=math.pi),
}
ISTFTNET_S_POST = {"1": 0.25, "2": 0.15}       # conv_post's weight scale by block type (type "2" stages end louder)
ISTFTNET_LOG_MAG = (-2.5, 1.5)                  # conv_post's bias on the log-magnitude channels: a ramp from DC to Nyquist
ISTFTNET_SIN_ARG = (-2.2, 2.2)                 # and on the phase channels


def make_istftnet_state_dict(dims=ISTFTNET_DIMS["c8c8i"], seed: int = SEED, weight_norm: Optional[str] = None) -> dict[str, torch.Tensor]:
    """Synthetic iSTFTNet generator weights in the official state-dict layout (HiFi-GAN's names, conv_post with n_fft + 2
    output channels), from keyed streams: make_hifigan_state_dict's scales up to the last stage, conv_post N(0, s^2 / (7 C))
    with s = ISTFTNET_S_POST[block type].  The last stage's rms grows several-fold from a one-frame mel to a long one, so the
    spread that exercises exp and sin is put into conv_post's bias, which no input can take away: N(0, 0.05^2) plus a ramp
    over the n_fft / 2 + 1 log-magnitude channels (ISTFTNET_LOG_MAG) and one over the phase channels (ISTFTNET_SIN_ARG).  On
    make_vocoder_mel, per utterance (tests/test_istftnet_host.py asserts it for every case the GPU tests use): the
    log-magnitudes span more than 4 units inside [-7, 4] (exp runs from below 0.1 to above 4), the argument of sin passes
    -pi / 2 and +pi / 2, and the waveform peaks between 0.1 and 4 with an rms above 0.04.  weight_norm: see
    _make_generator."""
    N = dims["gen_istft_n_fft"]
    sd = _make_generator("isn", dims, seed, weight_norm, 1.0, 1.4, {"1": (1.4, 0.5), "2": (0.7,)},
                         ISTFTNET_S_POST[str(dims["resblock"])], post_channels=N + 2)
    ramp = lambda lo_hi: torch.linspace(lo_hi[0], lo_hi[1], N // 2 + 1)
    sd["conv_post.bias"] += torch.cat([ramp(ISTFTNET_LOG_MAG), ramp(ISTFTNET_SIN_ARG)])
    return sd


# name -> generator configuration (bigvgan.BigVGan's constructor arguments).  "base": the published 22.05 kHz base model.
# "odd" / "odd2": HIFIGAN_DIMS["odd"]'s geometry with AMPBlock "1" / "2", plain snake without logscale, no bias in conv_post
# and a clamp in place of the final tanh.
BIGVGAN_DIMS = {
    "base": dict(n_mels=80, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                 resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3,
                 activation="snakebeta", snake_logscale=True, use_bias_at_final=True, use_tanh_at_final=True),
    "odd": dict(n_mels=20, upsample_initial_channel=128, upsample_rates=(3, 2), upsample_kernel_sizes=(7, 4),
                resblock="1", resblock_kernel_sizes=(3, 11), resblock_dilation_sizes=((1, 3, 5),) * 2,
                activation="snake", snake_logscale=False, use_bias_at_final=False, use_tanh_at_final=False),
    "odd2": dict(n_mels=20, upsample_initial_channel=128, upsample_rates=(3, 2), upsample_kernel_sizes=(7, 4),
                 resblock="2", resblock_kernel_sizes=(3, 11), resblock_dilation_sizes=((1, 3), (2, 5)),
                 activation="snake", snake_logscale=False, use_bias_at_final=False, use_tanh_at_final=False),
}


def bigvgan_filter() -> torch.Tensor:
    """The anti-aliasing low-pass of BigVGAN's activations, float64 [12]: 0.5 kaiser_window(12, beta) sinc(0.5 (j - 5.5)) with
    beta = 0.1102 (A - 8.7), A = 2.285 * 5 * pi * 1.2 + 7.95, normalised to sum 1."""
    beta = 0.1102 * (2.285 * 5 * math.pi * 1.2 + 7.95 - 8.7)
    j = torch.arange(12, dtype=torch.float64)
    f = 0.5 * torch.kaiser_window(12, periodic=False, beta=beta, dtype=torch.float64) * torch.sinc(0.5 * (j - 5.5))
    return f / f.sum()


def make_bigvgan_state_dict(dims=BIGVGAN_DIMS["base"], seed: int = SEED, weight_norm: Optional[str] = None) -> dict[str, torch.Tensor]:
    """Synthetic BigVGAN generator weights in the official state-dict layout (ups.{i}.0, resblocks.{n}.activations.{l}.act.alpha
    / beta, the filter buffers, activation_post), from keyed streams.  Convolution weights are N(0, s^2 / (C_in k)) with s = 1
    (first convolution of a type "1" unit), 0.5 (second), 0.7 (type "2"), up-convolutions N(0, 1 / (C_in k / stride)), biases
    N(0, 0.05^2): the activations' inputs have an rms around 1.  al is log-uniform in [1, 6] and B in [1, 4] (stored as their
    logarithms with snake_logscale), so al |u| lies around 1 to 10.  conv_post is scaled for output peaks of 0.2 - 0.9 under a
    final tanh, and so that a few per cent of the samples clamp on either side without one.  The filters are bigvgan_filter().
    weight_norm: see _make_generator."""
    beta, logscale = dims.get("activation", "snakebeta") == "snakebeta", dims.get("snake_logscale", True)
    filt = bigvgan_filter().float().reshape(1, 1, 12)

    def act(sd: dict, name: str, C: int):
        for key, lo, hi in (("alpha", 1.0, 6.0),) + ((("beta", 1.0, 4.0),) if beta else ()):
            v = np.exp(_rng(f"bvg/{name}.{key}", seed).uniform(math.log(lo), math.log(hi), size=(C,)))
            sd[f"{name}.act.{key}"] = torch.from_numpy((np.log(v) if logscale else v).astype(np.float32))
        sd[name + ".upsample.filter"] = filt.clone()
        sd[name + ".downsample.lowpass.filter"] = filt.clone()

    return _make_generator("bvg", dims, seed, weight_norm, 0.25, 1.0, {"1": (1.0, 0.5), "2": (0.7,)},
                           0.1 if dims.get("use_tanh_at_final", True) else 0.6, up_key="ups.{i}.0", act=act,
                           post_bias=dims.get("use_bias_at_final", True))


# ---------------------------------------------------------------------------------------------------- dataset statistics
# Batches for data.DatasetStats (tests/golden/dataset_stats.npz holds the reference's results on them): pitch in Hz as the
# extractor delivers it with mean 0 / std 1 - the discrete values fl(fl(1 / tau) * 22050), tau in 27 .. 524, 0 on unvoiced
# frames and on the trailing frame of dataset.py:152 - and a smooth positive energy.
STATS_CASES = ("voices", "mostly_unvoiced", "constant", "single_frame", "nan", "empty_len")
STATS_MAX_FRAMES = 1723          # the data bound of the recipe (441,088 samples at hop 256)


def stats_bounds(v: np.ndarray):
    """float64 (p25, p75, lower, upper) of remove_outliers (functions.py:27-32) on one utterance's values: the
    linear-interpolation quantiles at q (n - 1) of the sorted values and the 1.5 IQR fences."""
    s = np.sort(v.astype(np.float64))
    n = len(s)

    def quant(r4):                      # position r4 / 4
        lo = r4 // 4
        return s[lo] + 0.25 * (r4 % 4) * (s[min(lo + 1, n - 1)] - s[lo])

    p25, p75 = quant(n - 1), quant(3 * (n - 1))
    return p25, p75, p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)


def stats_margin_ok(v: np.ndarray) -> bool:
    """Whether the keep / drop decision of every value is the same in fp32 and float64 arithmetic: IQR == 0 (the fences are
    exact in any precision), or no value within 2^-20 (|p25| + |p75|) of a fence."""
    if len(v) == 0 or np.isnan(v).any():
        return True
    p25, p75, lower, upper = stats_bounds(v)
    if p75 == p25:
        return True
    eps = 2.0 ** -20 * (abs(p25) + abs(p75))
    x = v.astype(np.float64)
    return bool((np.abs(x - lower) > eps).all() and (np.abs(x - upper) > eps).all())


def _stats_utterance(g: np.random.Generator, frames: int, unvoiced: float):
    """One utterance: (pitch fp32 [frames], energy fp32 [frames]).  `unvoiced`: the fraction of unvoiced frames, in runs."""
    f32 = np.float32
    t = np.arange(frames)
    tau = g.uniform(70.0, 260.0) * np.exp(0.25 * np.sin(2 * np.pi * t / g.uniform(40.0, 160.0) + g.uniform(0, 2 * np.pi))
                                          + 0.02 * np.cumsum(g.standard_normal(frames)) / np.sqrt(np.maximum(t, 1)))
    tau = np.clip(np.rint(tau), 27, 524)
    jumps = g.random(frames) < 0.02                                 # octave errors: half or double the lag
    tau = np.where(jumps, np.clip(np.where(g.random(frames) < 0.5, np.rint(tau / 2), tau * 2), 27, 524), tau)
    hz = (f32(1) / tau.astype(f32)) * f32(22050)
    voiced = np.ones(frames, dtype=bool)
    want = int(round(unvoiced * frames))
    while frames and (~voiced).sum() < want:
        a = int(g.integers(0, frames))
        voiced[a:a + int(g.integers(1, 12))] = False
    if want < frames:                                               # trim the runs back to exactly `want` unvoiced frames
        off = np.flatnonzero(~voiced)
        voiced[off[want:]] = True
    pitch = np.where(voiced, hz, f32(0)).astype(f32)
    if frames:
        pitch[-1] = 0                                               # the pad of dataset.py:152
    energy = 3.0 + 1.2 * np.sin(2 * np.pi * t / g.uniform(30.0, 90.0) + g.uniform(0, 2 * np.pi)) + 0.15 * g.standard_normal(frames)
    energy = np.where(g.random(frames) < 0.01, energy + g.uniform(4.0, 8.0), energy)      # a few bursts above the fence
    return pitch, np.maximum(energy, 0.05).astype(f32)


def make_stats_case(case: str, seed: int = SEED) -> dict[str, torch.Tensor]:
    """{"pitch": fp32 [B, M], "energy": fp32 [B, M], "mel_len": int64 [B]}, zero past each mel_len.  Every utterance satisfies
    stats_margin_ok (one that does not is redrawn from the same stream), so kept counts are comparable exactly across
    precisions.  "voices": B = 64, lengths up to 1,723, 5-60 % unvoiced; "mostly_unvoiced": 75 % or more unvoiced (no pitch is
    kept) beside one ordinary utterance; "constant": a constant energy, a constant pitch, both; "single_frame": mel_len 1;
    "nan": a NaN in one utterance's pitch and in another's energy; "empty_len": mel_len 0."""
    if case not in STATS_CASES:
        raise ValueError(f"unknown stats case {case!r}")
    g = _rng(f"stats/{case}", seed)
    if case == "voices":
        lens = [STATS_MAX_FRAMES, 2] + [int(v) for v in g.integers(40, STATS_MAX_FRAMES, 62)]
        unv = [float(v) for v in g.uniform(0.05, 0.6, 64)]
    elif case == "mostly_unvoiced":
        lens, unv = [400, 401, 333, 512, 250], [0.75, 0.8, 0.95, 1.0, 0.3]
    elif case == "constant":
        lens, unv = [300, 200, 150, 280], [0.2, 0.0, 0.0, 0.4]
    elif case == "single_frame":
        lens, unv = [1, 1, 240], [0.0, 0.0, 0.3]
    elif case == "nan":
        lens, unv = [200, 300, 260], [0.3, 0.2, 0.25]
    else:
        lens, unv = [0, 180, 0], [0.0, 0.3, 0.0]
    M = max(lens)
    pitch, energy = np.zeros((len(lens), M), np.float32), np.zeros((len(lens), M), np.float32)
    for b, (n, u) in enumerate(zip(lens, unv)):
        for _ in range(16):
            p, e = _stats_utterance(g, n, u)
            if case == "constant":
                if b in (0, 2):
                    e[:] = np.float32(2.5)
                if b in (1, 2):
                    p[:] = np.float32(1) / np.float32(110) * np.float32(22050)       # (no trailing 0 either: IQR 0 at 200.45 Hz)
            if case == "nan" and b == 0:
                p[n // 3] = np.nan
            if case == "nan" and b == 1:
                e[n // 2] = np.nan
            if stats_margin_ok(p) and stats_margin_ok(e):
                break
        else:
            raise AssertionError(f"stats/{case}[{b}]: no draw with a safe margin")
        pitch[b, :n], energy[b, :n] = p, e
    return {"pitch": torch.from_numpy(pitch), "energy": torch.from_numpy(energy),
            "mel_len": torch.tensor(lens, dtype=torch.int64)}
