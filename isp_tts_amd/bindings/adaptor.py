"""Around the stacks (csrc/mas.hip, aligner.hip, glue.hip, hard_duration.hip): MAS, aligner, flow, embeddings, length regulators."""
from typing import Optional

import torch
from torch import Tensor

from .. import runtime as _rt

__all__ = ["mas", "pad_rows", "conv5_padded", "masked_instnorm", "aligner_scores", "soft_average", "flow_mix", "flow_finish",
           "flow_head", "flow_euler", "infer_features", "infer_features_items", "infer_features_tokens", "embed_tokens", "embed_tokens_qkv", "_speaker_ids", "add_speaker_",
           "add_speaker", "speaker_grad", "time_embedding", "length_regulate", "_hard_durations", "hard_regulate",
           "hard_regulate_bwd", "hard_average"]


# ------------------------------------------------------------------------------------------------- MAS
def mas(logits: Tensor, text_len: Tensor, mel_len: Tensor, want_dur: bool = True, want_path: bool = False):
    """ispk_mas_f32.  logits fp32 [B,M,L] (unit stride on L), lengths int64 [B] on the same device.
    Returns (attn_hard int16 [B,M,L], dur int64 [B,L] | None, path int16 [B,M] | None)."""
    _rt._dev(logits, text_len, mel_len)
    assert logits.dtype == torch.float32 and logits.ndim == 3
    if logits.stride(2) != 1:
        logits = logits.contiguous()
    B, M, L = logits.shape
    text_len = _rt._i64(text_len)
    mel_len = _rt._i64(mel_len)
    hard = torch.empty((B, M, L), dtype=torch.int16, device=logits.device)
    dur = torch.empty((B, L), dtype=torch.int64, device=logits.device) if want_dur else None
    path = torch.empty((B, M), dtype=torch.int16, device=logits.device) if want_path else None
    _rt._launch(f"mas_kernel<{(L + 63) // 64}>", 0.0, 6.0 * B * M * L, _rt.lib().ispk_mas_f32, logits.data_ptr(),
                text_len.data_ptr(), mel_len.data_ptr(), hard.data_ptr(), _rt._ptr(dur), _rt._ptr(path), B, M, L, logits.stride(0),
                logits.stride(1), _rt._stream())
    return hard, dur, path


# ------------------------------------------------------------------------------------------------- aligner front-end
def pad_rows(x: Tensor, lengths: Tensor, channel_first: bool = False, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_pad_rows_f32: [B,T,C] (or [B,C,T] with channel_first) -> masked, zero-padded channel-last [B,T+4,C]."""
    _rt._dev(x, lengths)
    assert x.dtype == torch.float32 and x.ndim == 3
    if channel_first:
        B, C, T = x.shape
        sb, sc, st = x.stride()
    else:
        B, T, C = x.shape
        sb, st, sc = x.stride()
    lengths = _rt._i64(lengths)
    split = out_dtype == torch.float16      # split fp16 planes [2, B, T+4, C] (hi, lo): the split-fp16 GEMMs' operand format
    out = torch.empty((2, B, T + 4, C) if split else (B, T + 4, C), dtype=out_dtype, device=x.device)
    _rt._launch("pad_rows_kernel", 0.0, 8.0 * B * T * C, _rt.lib().ispk_pad_rows_f32, x.data_ptr(), sb, st, sc,
                lengths.data_ptr(), out.data_ptr(), 2 if split else int(out_dtype == torch.bfloat16), B, T, C, _rt._stream())
    return out


def conv5_padded(xpad: Tensor, w2d: Tensor, flags: int = 0) -> Tensor:
    """Conv1d(kernel k, padding (k-1)/2, no bias) over a padded channel-last buffer as ONE GEMM over overlapping rows.
    xpad [B, T+4, C]; w2d [O, k*C] (= conv.weight.permute(0,2,1).reshape(O, k*C)), k = 5 or 1.  Returns [B, T+4, O] whose
    row t (not t+2) of every utterance is frame t; the last 4 rows per utterance are scratch."""
    _rt._dev(xpad, w2d)
    B, TP, C = xpad.shape
    O, K = w2d.shape
    taps = K // C
    assert taps * C == K and taps in (1, 5) and xpad.is_contiguous() and w2d.is_contiguous()
    assert xpad.dtype == w2d.dtype
    bf16 = xpad.dtype == torch.bfloat16
    out = torch.empty((B, TP, O), dtype=torch.float32, device=xpad.device)      # fp32 out on both paths
    a_ptr = xpad.data_ptr() + (0 if taps == 5 else 2 * C * xpad.element_size())  # k=1: frame t sits at padded row t+2
    M = B * TP - 4
    fn = _rt.lib().ispk_gemm_bf16 if bf16 else _rt.lib().ispk_gemm_f32
    _rt._launch(_rt._gemm_label(bf16, M, O, K), 2.0 * M * O * K, float(xpad.element_size()) * (M * C + O * K) + 4.0 * M * O, fn,
                a_ptr, C, w2d.data_ptr(), K, out.data_ptr(), O, None, None, 0, None, M, O, K, flags, 0, 0, _rt._stream())
    return out


def masked_instnorm(y: Tensor, weight: Tensor, bias: Tensor, lengths: Tensor, eps: float = 1e-5,
                    out_dtype: torch.dtype = torch.float32) -> Tensor:
    """ispk_masked_instnorm_f32: conv output [B,T+4,C] (row t = frame t) -> normalised, masked, re-padded [B,T+4,C]."""
    _rt._dev(y, weight, bias, lengths)
    B, TP, C = y.shape
    split = out_dtype == torch.float16      # split fp16 planes [2, B, T+4, C]
    out = torch.empty((2, *y.shape) if split else y.shape, dtype=out_dtype, device=y.device)
    lengths = _rt._i64(lengths)
    _rt._launch("masked_instnorm_kernel", 0.0, 16.0 * B * TP * C, _rt.lib().ispk_masked_instnorm_f32, y.data_ptr(),
                weight.data_ptr(), bias.data_ptr(), lengths.data_ptr(), out.data_ptr(), 2 if split else int(out_dtype == torch.bfloat16), B,
                TP - 4, C, eps, _rt._stream())
    return out


def aligner_scores(q_enc: Tensor, k_enc: Tensor, text_len: Tensor, mel_len: Tensor, M: int, L: int, fast: bool = False):
    """ispk_aligner_scores_f32: q_enc [B, M+4, 128], k_enc [B, L+4, 128] (row t = frame/token t) ->
    (attn_soft, attn_logits), both [B, M, L].  `fast`: ispk_aligner_scores_fast_f32 (bf16 compute path: split-bf16 score
    products, hardware exp / log)."""
    _rt._dev(q_enc, k_enc, text_len, mel_len)
    B, D = q_enc.shape[0], q_enc.shape[2]
    logits = torch.empty((B, M, L), dtype=torch.float32, device=q_enc.device)
    soft = torch.empty((B, M, L), dtype=torch.float32, device=q_enc.device)
    text_len = _rt._i64(text_len)
    mel_len = _rt._i64(mel_len)
    _rt._launch("aligner_scores_kernel<bf16x3>" if fast else "aligner_scores_kernel", 2.0 * B * M * L * D, 4.0 * B * (M * D + L * D + 2 * M * L),
                _rt.lib().ispk_aligner_scores_fast_f32 if fast else _rt.lib().ispk_aligner_scores_f32, q_enc.data_ptr(), q_enc.stride(0),
                k_enc.data_ptr(), k_enc.stride(0), text_len.data_ptr(), mel_len.data_ptr(), logits.data_ptr(), soft.data_ptr(), B, M, L, D,
                _rt._stream())
    return soft, logits


def soft_average(attn_soft: Tensor, pitch: Tensor, energy: Tensor, duration: Optional[Tensor], text_len: Tensor) -> Tensor:
    """ispk_soft_average_f32 -> feats [B, L, 3] = (log1p(duration) - or 0 without durations -, pitch target, energy target)."""
    _rt._dev(attn_soft, pitch, energy, duration, text_len)
    B, M, L = attn_soft.shape
    feats = torch.empty((B, L, 3), dtype=torch.float32, device=attn_soft.device)
    dur = _rt._i64(duration)
    if B == 0:      # nothing to compute; the C entries would refuse the NULL data_ptr() torch gives an empty tensor
        return feats
    _rt._launch("soft_average_kernel", 0.0, 4.0 * B * M * L, _rt.lib().ispk_soft_average_f32, attn_soft.contiguous().data_ptr(),
                pitch.contiguous().data_ptr(), energy.contiguous().data_ptr(), _rt._ptr(dur),
                _rt._i64(text_len).data_ptr(), feats.data_ptr(), B, M, L, _rt._stream())
    return feats


def flow_mix(x0: Tensor, x1: Tensor, t: Tensor, sigma: float):
    """ispk_flow_mix_f32 -> (x_t, flow), both [B, L, C] fp32."""
    _rt._dev(x0, x1, t)
    B, L, C = x1.shape
    x0c, x1c, tc = x0.float().contiguous(), x1.float().contiguous(), t.float().contiguous()
    xt, flow = torch.empty_like(x1c), torch.empty_like(x1c)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        return xt, flow
    _rt._launch("flow_mix_kernel", 0.0, 16.0 * B * L * C, _rt.lib().ispk_flow_mix_f32, x0c.data_ptr(), x1c.data_ptr(), tc.data_ptr(),
                float(sigma), xt.data_ptr(), flow.data_ptr(), B, L, C, _rt._stream())
    return xt, flow


def flow_finish(pred_raw: Tensor, flow: Tensor, x0: Tensor, mask: Tensor):
    """ispk_flow_finish_f32 -> (pred [B,L,C], duration [B,L], loss_ratio [B], loss = mean(loss_ratio) 0-d)."""
    _rt._dev(pred_raw, flow, x0, mask)
    B, L, C = pred_raw.shape
    assert mask.dtype == torch.bool and mask.shape == (B, L)
    pr, fl, x0c, mk = pred_raw.float().contiguous(), flow.contiguous(), x0.float().contiguous(), mask.contiguous()
    pred = torch.empty_like(pr)
    dur = torch.empty((B, L), dtype=torch.float32, device=pr.device)
    ratio = torch.empty((B,), dtype=torch.float32, device=pr.device)
    loss = torch.empty((), dtype=torch.float32, device=pr.device)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average); the mean over no utterance is NaN, as torch's is
        return pred, dur, ratio, loss.fill_(float("nan"))
    _rt._launch("flow_finish_kernel", 0.0, 20.0 * B * L * C, _rt.lib().ispk_flow_finish_f32, pr.data_ptr(), fl.data_ptr(),
                x0c.data_ptr(), mk.data_ptr(), pred.data_ptr(), dur.data_ptr(), ratio.data_ptr(), loss.data_ptr(), B, L, C,
                _rt._stream())
    return pred, dur, ratio, loss


def flow_head(y: Tensor, norm_weight: Tensor, norm_bias: Tensor, norm_eps: float, weight: Tensor, bias: Tensor, flow: Tensor,
              x0: Tensor, mask: Tensor):
    """ispk_flow_head_f32: the predictor's final LayerNorm (row-masked) + 256 -> 3 linear_layer + `flow_finish` on the stack's raw
    output rows y [B, L, 256] -> (pred [B,L,3], duration [B,L], loss_ratio [B], loss 0-d), two launches instead of three."""
    _rt._dev(y, norm_weight, norm_bias, weight, bias, flow, x0, mask)
    B, L, D = y.shape
    C = weight.shape[0]
    assert y.dtype == torch.float32 and y.stride(2) == 1 and y.stride(0) == L * y.stride(1) and weight.shape == (C, D) and weight.is_contiguous()
    assert mask.dtype == torch.bool and mask.shape == (B, L)
    fl, x0c, mk = flow.contiguous(), x0.float().contiguous(), mask.contiguous()
    pred = torch.empty((B, L, C), dtype=torch.float32, device=y.device)
    dur = torch.empty((B, L), dtype=torch.float32, device=y.device)
    ratio = torch.empty((B,), dtype=torch.float32, device=y.device)
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average); the mean over no utterance is NaN, as torch's is
        return pred, dur, ratio, loss.fill_(float("nan"))
    ws = torch.empty((2 * B * ((L + 15) // 16),), dtype=torch.float32, device=y.device)
    _rt._launch("flow_head_kernels", 0.0, 4.0 * B * L * D, _rt.lib().ispk_flow_head_f32, y.data_ptr(), y.stride(1), norm_weight.data_ptr(),
                norm_bias.data_ptr(), float(norm_eps), weight.data_ptr(), bias.data_ptr(), fl.data_ptr(), x0c.data_ptr(), mk.data_ptr(),
                pred.data_ptr(), dur.data_ptr(), ratio.data_ptr(), loss.data_ptr(), ws.data_ptr(), B, L, D, C, _rt._stream())
    return pred, dur, ratio, loss


def flow_euler(x_t: Tensor, velocity: Tensor, dt: float, mask: Optional[Tensor] = None) -> Tensor:
    """ispk_flow_euler_f32: x_t + velocity * dt [* mask[..., None]] (one Euler step of the flow predictor's `infer`)."""
    _rt._dev(x_t, velocity, mask)
    B, L, C = x_t.shape
    xc, vc = x_t.float().contiguous(), velocity.float().contiguous()
    out = torch.empty_like(xc)
    if mask is not None:
        mask = mask.contiguous()
        assert mask.dtype == torch.bool and mask.shape == (B, L)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        return out
    _rt._launch("flow_euler_kernel", 0.0, 12.0 * B * L * C, _rt.lib().ispk_flow_euler_f32, xc.data_ptr(), vc.data_ptr(), float(dt),
                _rt._ptr(mask), out.data_ptr(), B, L, C, _rt._stream())
    return out


def infer_features(pred: Tensor, duration_target: Optional[Tensor], pitch_target: Optional[Tensor],
                   energy_target: Optional[Tensor], duration_factor: float = 1.0, pitch_factor: float = 1.0,
                   pitch_delta: float = 0.0, energy_factor: float = 1.0, energy_delta: float = 0.0, round_duration: bool = False):
    """ispk_infer_features_f32: pred [B, L, 3] -> (duration fp32 [B, L], features fp32 [B, L, 2]).  `round_duration` (hard
    durations): ispk_infer_features_round_f32, the predicted durations rounded half to even before the clamp."""
    _rt._dev(pred, duration_target, pitch_target, energy_target)
    B, L, C = pred.shape
    assert C == 3 and pred.dtype == torch.float32
    pc = pred.contiguous()
    dur_f = dur_i = None
    if duration_target is not None:
        assert duration_target.shape == (B, L)
        if duration_target.dtype == torch.int64:
            dur_i = duration_target.contiguous()
        else:
            dur_f = duration_target.float().contiguous()
    pt = None if pitch_target is None else pitch_target.float().reshape(B, L).contiguous()
    et = None if energy_target is None else energy_target.float().reshape(B, L).contiguous()
    duration = torch.empty((B, L), dtype=torch.float32, device=pred.device)
    feats = torch.empty((B, L, 2), dtype=torch.float32, device=pred.device)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        return duration, feats
    _rt._launch("infer_features_kernel<round>" if round_duration else "infer_features_kernel", 0.0, 24.0 * B * L,
                _rt.lib().ispk_infer_features_round_f32 if round_duration else _rt.lib().ispk_infer_features_f32, pc.data_ptr(), _rt._ptr(dur_f),
                _rt._ptr(dur_i), _rt._ptr(pt), _rt._ptr(et), float(duration_factor), float(pitch_factor), float(pitch_delta), float(energy_factor),
                float(energy_delta), duration.data_ptr(), feats.data_ptr(), B, L, _rt._stream())
    return duration, feats


def infer_features_items(pred: Tensor, duration_target: Optional[Tensor], pitch_target: Optional[Tensor],
                         energy_target: Optional[Tensor], controls: Tensor, round_duration: bool = False,
                         want_frames: bool = True):
    """ispk_infer_features_items_f32: `infer_features` with one control row per utterance, controls fp32 [B, 5] on the device =
    (duration_factor, pitch_factor, pitch_delta, energy_factor, energy_delta) -> (duration fp32 [B, L], features fp32 [B, L, 2],
    frames_wanted int64 [B] | None: the decoder length the regulator reports for these durations when nothing clamps it)."""
    _rt._dev(pred, duration_target, pitch_target, energy_target, controls)
    B, L, C = pred.shape
    assert C == 3 and pred.dtype == torch.float32
    if controls.dtype != torch.float32 or tuple(controls.shape) != (B, 5):
        raise ValueError(f"controls: fp32 [{B}, 5], got {controls.dtype} {tuple(controls.shape)}")
    pc, cc = pred.contiguous(), controls.contiguous()
    dur_f = dur_i = None
    if duration_target is not None:
        assert duration_target.shape == (B, L)
        if duration_target.dtype == torch.int64:
            dur_i = duration_target.contiguous()
        else:
            dur_f = duration_target.float().contiguous()
    pt = None if pitch_target is None else pitch_target.float().reshape(B, L).contiguous()
    et = None if energy_target is None else energy_target.float().reshape(B, L).contiguous()
    duration = torch.empty((B, L), dtype=torch.float32, device=pred.device)
    feats = torch.empty((B, L, 2), dtype=torch.float32, device=pred.device)
    frames = torch.empty((B,), dtype=torch.int64, device=pred.device) if want_frames else None
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        return duration, feats, frames
    _rt._launch("infer_features_items_kernel<round>" if round_duration else "infer_features_items_kernel", 0.0, 24.0 * B * L,
                _rt.lib().ispk_infer_features_items_f32, pc.data_ptr(), _rt._ptr(dur_f), _rt._ptr(dur_i), _rt._ptr(pt), _rt._ptr(et),
                cc.data_ptr(), int(bool(round_duration)), duration.data_ptr(), feats.data_ptr(), _rt._ptr(frames), B, L, _rt._stream())
    return duration, feats, frames


def infer_features_tokens(pred: Tensor, duration_target: Optional[Tensor], pitch_target: Optional[Tensor],
                          energy_target: Optional[Tensor], controls: Tensor, round_duration: bool = False,
                          want_frames: bool = True):
    """ispk_infer_features_tokens_f32: `infer_features_items` with one control row per TOKEN, controls fp32 [B, L, 5] on the
    device.  Rows that are constant over an utterance give the bits of `infer_features_items`."""
    _rt._dev(pred, duration_target, pitch_target, energy_target, controls)
    B, L, C = pred.shape
    assert C == 3 and pred.dtype == torch.float32
    if controls.dtype != torch.float32 or tuple(controls.shape) != (B, L, 5):
        raise ValueError(f"controls: fp32 [{B}, {L}, 5], got {controls.dtype} {tuple(controls.shape)}")
    pc, cc = pred.contiguous(), controls.contiguous()
    dur_f = dur_i = None
    if duration_target is not None:
        assert duration_target.shape == (B, L)
        if duration_target.dtype == torch.int64:
            dur_i = duration_target.contiguous()
        else:
            dur_f = duration_target.float().contiguous()
    pt = None if pitch_target is None else pitch_target.float().reshape(B, L).contiguous()
    et = None if energy_target is None else energy_target.float().reshape(B, L).contiguous()
    duration = torch.empty((B, L), dtype=torch.float32, device=pred.device)
    feats = torch.empty((B, L, 2), dtype=torch.float32, device=pred.device)
    frames = torch.empty((B,), dtype=torch.int64, device=pred.device) if want_frames else None
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        return duration, feats, frames
    _rt._launch("infer_features_tokens_kernel<round>" if round_duration else "infer_features_tokens_kernel", 0.0, 44.0 * B * L,
                _rt.lib().ispk_infer_features_tokens_f32, pc.data_ptr(), _rt._ptr(dur_f), _rt._ptr(dur_i), _rt._ptr(pt), _rt._ptr(et),
                cc.data_ptr(), int(bool(round_duration)), duration.data_ptr(), feats.data_ptr(), _rt._ptr(frames), B, L, _rt._stream())
    return duration, feats, frames


# ------------------------------------------------------------------------------------------------- between the stacks
def embed_tokens(text: Tensor, table: Tensor, text_len: Optional[Tensor] = None, want_mask: bool = True):
    """ispk_embed_tokens_f32: (emb fp32 [B,L,D], mask bool [B,L] | None) - nn.Embedding lookup + the key mask."""
    _rt._dev(text, table, text_len)
    assert text.dtype == torch.int64 and text.ndim == 2 and table.dtype == torch.float32 and table.stride(1) == 1
    B, L = text.shape
    V, D = table.shape
    text = text.contiguous()
    emb = torch.empty((B, L, D), dtype=torch.float32, device=text.device)
    mask = torch.empty((B, L), dtype=torch.bool, device=text.device) if want_mask else None
    text_len = _rt._i64(text_len)
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        return emb, mask
    _rt._launch("embed_tokens_kernel", 0.0, 8.0 * B * L * D, _rt.lib().ispk_embed_tokens_f32, text.data_ptr(), table.data_ptr(),
                table.stride(0), V, _rt._ptr(text_len), emb.data_ptr(), _rt._ptr(mask), B, L, D, _rt._stream())
    return emb, mask


def embed_tokens_qkv(text: Tensor, table: Tensor, qkv_table: Tensor, text_len: Optional[Tensor] = None, want_mask: bool = True):
    """ispk_embed_tokens_qkv: `embed_tokens` plus the first layer's q/kv rows gathered with the same ids from `qkv_table` (bf16
    [vocab, N]: attention_norm + [to_q; to_kv] of every table row) -> (emb fp32 [B,L,D], mask bool [B,L] | None, qkv bf16 [B,L,N])."""
    _rt._dev(text, table, qkv_table, text_len)
    assert text.dtype == torch.int64 and text.ndim == 2 and table.dtype == torch.float32 and table.stride(1) == 1
    B, L = text.shape
    V, D = table.shape
    N = qkv_table.shape[1]
    assert qkv_table.dtype == torch.bfloat16 and qkv_table.shape == (V, N) and qkv_table.stride(1) == 1
    text = text.contiguous()
    emb = torch.empty((B, L, D), dtype=torch.float32, device=text.device)
    qkv = torch.empty((B, L, N), dtype=torch.bfloat16, device=text.device)
    mask = torch.empty((B, L), dtype=torch.bool, device=text.device) if want_mask else None
    text_len = _rt._i64(text_len)
    _rt._launch("embed_tokens_qkv_kernel", 0.0, B * L * (8.0 * D + 4.0 * N), _rt.lib().ispk_embed_tokens_qkv, text.data_ptr(),
                table.data_ptr(), table.stride(0), V, _rt._ptr(text_len), emb.data_ptr(), _rt._ptr(mask), qkv_table.data_ptr(),
                qkv_table.stride(0), qkv.data_ptr(), B, L, D, N, _rt._stream())
    return emb, mask, qkv


def _speaker_ids(speaker: Tensor, B: int):
    """-> (contiguous int64 ids, id_stride): `speaker` int64 [B, 1] (the collator's field, collator.py:59) = one id per utterance,
    or one element = one id for the whole batch (the notebook's `torch.tensor([id])`)."""
    assert speaker.dtype == torch.int64
    if speaker.numel() == 1:
        return speaker.contiguous(), 0
    if speaker.ndim == 2 and tuple(speaker.shape) == (B, 1):
        return speaker.contiguous(), 1
    raise ValueError(f"speaker of shape {tuple(speaker.shape)} does not broadcast against enc_out [B={B}, L, D] "
                     "(the reference takes [B, 1] ids or a single id)")


def add_speaker_(x: Tensor, table: Tensor, speaker: Tensor) -> Tensor:
    """ispk_add_speaker_f32: x [B, L, D] += table[speaker] in place, broadcast over L the way the reference's
    `enc_out + self.speaker_embedding(speaker)` broadcasts (model.py:205-207): `speaker` int64 [B, 1] (the collator's field,
    collator.py:59) = one id per utterance, or one element = one id for the whole batch (the notebook's `torch.tensor([id])`)."""
    _rt._dev(x, table, speaker)
    assert x.dtype == torch.float32 and x.ndim == 3 and x.is_contiguous() and table.dtype == torch.float32 and table.stride(1) == 1
    B, L, D = x.shape
    assert table.shape[1] == D
    speaker, stride = _speaker_ids(speaker, B)
    _rt._launch("add_speaker_kernel", 0.0, 8.0 * B * L * D, _rt.lib().ispk_add_speaker_f32, x.data_ptr(), table.data_ptr(), table.stride(0),
                table.shape[0], speaker.data_ptr(), stride, B, L, D, _rt._stream())
    return x


def add_speaker(x: Tensor, table: Tensor, speaker: Tensor) -> Tensor:
    """ispk_add_speaker_out_f32: -> x [B, L, D] + table[speaker] in a new tensor, bit for bit what `add_speaker_` leaves in
    place; x is untouched (the teacher-forced forward: the aligner reads - and its backward keeps - the un-added tensor)."""
    _rt._dev(x, table, speaker)
    assert x.dtype == torch.float32 and x.ndim == 3 and x.is_contiguous() and table.dtype == torch.float32 and table.stride(1) == 1
    B, L, D = x.shape
    assert table.shape[1] == D
    speaker, stride = _speaker_ids(speaker, B)
    out = torch.empty_like(x)
    _rt._launch("add_speaker_out_kernel", 0.0, 8.0 * B * L * D, _rt.lib().ispk_add_speaker_out_f32, x.data_ptr(), out.data_ptr(),
                table.data_ptr(), table.stride(0), table.shape[0], speaker.data_ptr(), stride, B, L, D, _rt._stream())
    return out


def speaker_grad(d_x: Tensor, speaker: Tensor, speakers: int, text_len: Optional[Tensor] = None, out: Optional[Tensor] = None,
                 accumulate: bool = False) -> Tensor:
    """ispk_speaker_grad_f32: d_x fp32 [B, L, D] -> d_table [speakers, D], row s the sum of d_x[b, :text_len[b]] over the
    utterances of speaker s (fixed order, no atomics); rows of absent speakers are zero.  `out` (contiguous [speakers, D]) is
    written, or - `accumulate` - added to."""
    _rt._dev(d_x, speaker, text_len, out)
    assert d_x.dtype == torch.float32 and d_x.ndim == 3
    d_x = d_x.contiguous()
    B, L, D = d_x.shape
    speaker, stride = _speaker_ids(speaker, B)
    if text_len is not None:
        text_len = _rt._i64(text_len)
        assert text_len.numel() == B
    if out is None:
        assert not accumulate
        out = torch.empty((speakers, D), dtype=torch.float32, device=d_x.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (speakers, D) and out.stride(1) == 1
    ws = _rt.workspace(d_x.device, B * -(-L // 16) * D)
    _rt._launch("speaker_grad_kernels", 1.0 * B * L * D, 4.0 * B * L * D + 4.0 * speakers * D, _rt.lib().ispk_speaker_grad_f32, d_x.data_ptr(),
                speaker.data_ptr(), stride, _rt._ptr(text_len), ws.data_ptr(), ws.numel(), out.data_ptr(), out.stride(0), speakers, B, L, D,
                1 if accumulate else 0, _rt._stream())
    return out


def time_embedding(t: Tensor, inv_freq: Tensor, freq_scale: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor) -> Tensor:
    """ispk_time_embedding_f32: t [...] -> [..., emb_dim] (sinusoid with the raw position, Linear, SiLU, Linear)."""
    _rt._dev(t, inv_freq, freq_scale, w0, b0, w1, b1)
    tf = t.to(torch.float32).contiguous()
    E, H = w1.shape[0], inv_freq.numel()
    assert w0.shape == (E, 1 + 2 * H) and w1.shape == (E, E) and w0.is_contiguous() and w1.is_contiguous()
    out = torch.empty((*t.shape, E), dtype=torch.float32, device=t.device)
    if tf.numel() == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        return out
    _rt._launch("time_embedding_kernel", 0.0, 0.0, _rt.lib().ispk_time_embedding_f32, tf.data_ptr(), tf.numel(), inv_freq.data_ptr(),
                freq_scale.data_ptr(), H, w0.data_ptr(), b0.data_ptr(), w1.data_ptr(), b1.data_ptr(), E, out.data_ptr(),
                _rt._stream())
    return out


def length_regulate(x: Tensor, durations: Tensor, alignment: Optional[Tensor], frames: int, max_len: int = -1,
                    enc_len: Optional[Tensor] = None, want_mask: bool = True, split_bf16=False, next_qkv: Optional[tuple] = None):
    """ispk_length_regulate_f32 -> (out fp32 [B, frames, D], dec_len int64 [B], dec_mask bool [B, frames] | None).
    alignment fp32 [B, frames, L] (forward), or None: the soft path generated from the fp32 `durations` (infer).
    `split_bf16`: True = ispk_length_regulate_split_bf16 (the bf16 compute path: three bf16 MFMAs per product, ~2^-16
    relative); "f16" = ispk_length_regulate_split_f16 (the split-fp16 parity path: fp16 terms, fp32-grade).
    `next_qkv` = (gamma, beta, eps, Wqkv_chunks) (bf16 path, D = 384; Wqkv_chunks from `chunk_k16`, [24, 512, 16]):
    ispk_length_regulate_qkv_bf16 - the same three outputs, bit for bit, and a fourth: the consuming layer's attention_norm +
    q/kv projection of every output row, bf16 [B, frames, 512], from the kernel's epilogue."""
    _rt._dev(x, durations, alignment, enc_len)
    assert x.dtype == torch.float32 and x.ndim == 3
    if x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        x = x.contiguous()
    B, L, D = x.shape
    if alignment is not None:
        assert alignment.dtype == torch.float32 and alignment.shape == (B, frames, L)
        alignment = alignment.contiguous()
    dur_f = dur_i = None
    dur_cols = L
    if durations.dtype == torch.int64:   # only summed: any [B, cols] with the right row sums (e.g. mel_len as [B, 1])
        assert alignment is not None, "the soft path is generated from fp32 durations"
        dur_i = durations.reshape(B, -1 if B else max(durations.shape[-1], 1)).contiguous()      # (-1 is ambiguous with no rows)
        dur_cols = dur_i.shape[1]
    else:
        dur_f = durations.to(torch.float32).contiguous()
        assert dur_f.shape == (B, L)
    enc_len = _rt._i64(enc_len)
    out = torch.empty((B, frames, D), dtype=torch.float32, device=x.device)
    dec_len = torch.empty((B,), dtype=torch.int64, device=x.device)
    mask = torch.empty((B, frames), dtype=torch.bool, device=x.device) if want_mask else None
    nb = 4.0 * B * (frames * D + L * D + (frames * L if alignment is not None else 0))
    if B == 0:      # (NULL data_ptr() of an empty tensor: see soft_average)
        qkv = () if next_qkv is None else (torch.empty((B, frames, 512), dtype=torch.bfloat16, device=x.device),)
        return (out, dec_len, mask, *qkv)
    if next_qkv is not None:
        gamma, beta, eps, wqc = next_qkv
        _rt._dev(gamma, beta, wqc)
        assert split_bf16 is True and D == 384, "the q/kv epilogue is built for the bf16 path at dim 384"
        assert wqc.dtype == torch.bfloat16 and wqc.shape == (D // 16, 512, 16) and wqc.is_contiguous()
        assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == D
        qkv = torch.empty((B, frames, 512), dtype=torch.bfloat16, device=x.device)
        _rt._launch("length_regulate_qkv_kernel", 2.0 * B * frames * (L + 512) * D, nb + 2.0 * (B * frames * 512 + 512 * D),
                    _rt.lib().ispk_length_regulate_qkv_bf16, _rt._ptr(alignment), _rt._ptr(dur_f), _rt._ptr(dur_i), _rt._ptr(enc_len), x.data_ptr(),
                    x.stride(1), out.data_ptr(), dec_len.data_ptr(), _rt._ptr(mask), gamma.data_ptr(), beta.data_ptr(), float(eps),
                    wqc.data_ptr(), qkv.data_ptr(), 512, B, frames, L, D, max_len, dur_cols, _rt._stream())
        return out, dec_len, mask, qkv
    fn = (_rt.lib().ispk_length_regulate_split_f16 if split_bf16 == "f16" else
          _rt.lib().ispk_length_regulate_split_bf16 if split_bf16 else _rt.lib().ispk_length_regulate_f32)
    _rt._launch("length_regulate_kernel<split_f16>" if split_bf16 == "f16" else "length_regulate_kernel<bf16x3>" if split_bf16
                else "length_regulate_kernel", 2.0 * B * frames * L * D, nb, fn, _rt._ptr(alignment),
                _rt._ptr(dur_f), _rt._ptr(dur_i), _rt._ptr(enc_len), x.data_ptr(), x.stride(1), out.data_ptr(), dec_len.data_ptr(),
                _rt._ptr(mask), B, frames, L, D, max_len, dur_cols, _rt._stream())
    return out, dec_len, mask


def _hard_durations(durations: Tensor, B: int, L: int):
    """-> (fp32 pointer source | None, int64 pointer source | None) of [B, L] durations: int64 (MAS) or fp32 (`infer`)."""
    assert durations.shape == (B, L), f"durations {tuple(durations.shape)}: one per token, [{B}, {L}]"
    if durations.dtype == torch.int64:
        return None, durations.contiguous()
    return durations.to(torch.float32).contiguous(), None


def hard_regulate(x: Tensor, durations: Tensor, frames: int, max_len: int = -1, want_mask: bool = True):
    """ispk_hard_regulate_f32 -> (out fp32 [B, frames, D], dec_len int64 [B], dec_mask bool [B, frames] | None): every token row
    of x [B, L, D] repeated (float(duration) + 0.5).long() times, zero rows behind the last one."""
    _rt._dev(x, durations)
    assert x.dtype == torch.float32 and x.ndim == 3
    if x.stride(2) != 1 or x.stride(0) != x.shape[1] * x.stride(1):
        x = x.contiguous()
    B, L, D = x.shape
    dur_f, dur_i = _hard_durations(durations, B, L)
    out = torch.empty((B, frames, D), dtype=torch.float32, device=x.device)
    dec_len = torch.empty((B,), dtype=torch.int64, device=x.device)
    mask = torch.empty((B, frames), dtype=torch.bool, device=x.device) if want_mask else None
    _rt._launch("hard_regulate_kernel", 0.0, 4.0 * B * D * (frames + L), _rt.lib().ispk_hard_regulate_f32, _rt._ptr(dur_f), _rt._ptr(dur_i),
                x.data_ptr(), x.stride(1), out.data_ptr(), dec_len.data_ptr(), _rt._ptr(mask), B, frames, L, D, max_len, _rt._stream())
    return out, dec_len, mask


def hard_regulate_bwd(d_out: Tensor, durations: Tensor, max_len: int = -1) -> Tensor:
    """ispk_hard_regulate_bwd_f32: d_out [B, rows, D] -> d_x [B, L, D], each token the sum of its frames' rows in frame order."""
    _rt._dev(d_out, durations)
    assert d_out.dtype == torch.float32 and d_out.ndim == 3
    d_out = d_out.contiguous()
    B, rows, D = d_out.shape
    L = durations.shape[1]
    dur_f, dur_i = _hard_durations(durations, B, L)
    d_x = torch.empty((B, L, D), dtype=torch.float32, device=d_out.device)
    _rt._launch("hard_regulate_bwd_kernel", 1.0 * B * rows * D, 4.0 * B * D * (rows + L), _rt.lib().ispk_hard_regulate_bwd_f32, _rt._ptr(dur_f),
                _rt._ptr(dur_i), d_out.data_ptr(), d_x.data_ptr(), B, rows, L, D, max_len, _rt._stream())
    return d_x


def hard_average(pitch: Tensor, energy: Tensor, duration: Tensor, text_len: Tensor) -> Tensor:
    """ispk_hard_average_f32 -> feats [B, L, 3] = (log1p(duration), mean of each token's non-zero pitch frames, same for energy);
    pitch / energy fp32 [B, M], duration int64 [B, L]."""
    _rt._dev(pitch, energy, duration, text_len)
    B, M = pitch.shape
    L = duration.shape[1]
    assert duration.dtype == torch.int64 and duration.shape == (B, L) and energy.shape == (B, M)
    feats = torch.empty((B, L, 3), dtype=torch.float32, device=pitch.device)
    # (copies of strided views stay referenced until the launch is queued: a freed one's block would be handed to the next copy)
    pc, ec, dc, tc = pitch.float().contiguous(), energy.float().contiguous(), duration.contiguous(), _rt._i64(text_len)
    _rt._launch("hard_average_kernel", 0.0, 8.0 * B * M + 20.0 * B * L, _rt.lib().ispk_hard_average_f32, pc.data_ptr(), ec.data_ptr(),
                dc.data_ptr(), tc.data_ptr(), feats.data_ptr(), B, M, L, _rt._stream())
    return feats
