"""Long-form synthesis: texts longer than one sentence, from the text to 16-bit PCM in ONE captured HIP graph.

The caller splits a text into sentences and buckets them; a bucket runs as a batch sorted for speed, not for reading.  Three
pieces put the documents back together on the device, with no host read:

    controls = make_controls(B, duration_factor=[1.0, 0.9, ...], pitch_delta=..., device=dev)   # one row per sentence
    mel, ao = model.infer(text, text_lengths=tl, controls=controls, max_dec_len=M, ...)         # read by the kernel
    r = join(audio, audio_len, doc, pos, pause, num_docs=D, out_samples=S_out, fade=64)          # r["audio"] fp32 [D, S_out]

and `Synthesizer` captures the whole chain - infer, vocoder, optional denoiser and trim, join, optional document loudness,
PCM16, optional speech marks - over static buffers.  `speech_marks` (csrc/marks.hip) says where every token and word lies in
an item or in its joined document; `cues` and `webvtt` turn word marks into subtitles on the host.  The join (csrc/join.hip; include/ispk.h has the arithmetic) orders the valid items by
(doc, pos, b), puts `pause[b]` samples of silence behind item b or - negative - crossfades it with its successor over
min(-pause, n / 2, n_next / 2) samples with weights that add up to one, and fades the remaining edges over `fade` samples.

Word-level prosody steers single words: `prosody_spans` turns SSML-like spans into per-token controls fp32 [B, L, 5] for
`infer(controls=)` and linear gains [B, L] for `gain_envelope` (csrc/prosody.hip), which scales every token's samples with short
linear ramps at the token boundaries; `Synthesizer(prosody=True)` has both in its captured chain.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch
from torch import Tensor

from . import graph, runtime
from .data.condition import AudioConditioner, Limiter, to_pcm16
from .data.equalize import Equalizer

CONTROL_NAMES = ("duration_factor", "pitch_factor", "pitch_delta", "energy_factor", "energy_delta")


def make_controls(B: int, duration_factor: Union[float, Sequence[float]] = 1.0, pitch_factor: Union[float, Sequence[float]] = 1.0,
                  pitch_delta: Union[float, Sequence[float]] = 0.0, energy_factor: Union[float, Sequence[float]] = 1.0,
                  energy_delta: Union[float, Sequence[float]] = 0.0, *, pitch_std: Optional[float] = None, device=None) -> Tensor:
    """fp32 [B, 5] for `infer(controls=)`: each argument a scalar or a sequence of B values.  `pitch_std` divides the
    pitch_delta column, as `infer(pitch_normalize=True)` does for the scalar."""
    cols = []
    for name, v in zip(CONTROL_NAMES, (duration_factor, pitch_factor, pitch_delta, energy_factor, energy_delta)):
        col = torch.as_tensor(v, dtype=torch.float64).detach().cpu()
        if col.ndim == 0:
            col = col.expand(B)
        if tuple(col.shape) != (B,):
            raise ValueError(f"{name}: a scalar or {B} values, got shape {tuple(col.shape)}")
        cols.append(col)
    if pitch_std is not None:
        cols[2] = cols[2] / float(pitch_std)
    return torch.stack(cols, dim=1).to(dtype=torch.float32, device=device)


def join_outputs(num_docs: int, out_samples: int, B: int, device) -> dict:
    """The tensors `join` fills, for a caller that keeps them (a graph capture)."""
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)      # noqa: E731
    return dict(audio=e((num_docs, out_samples), torch.float32), audio_len=e((num_docs,), torch.int64),
                wanted_len=e((num_docs,), torch.int64), item_offset=e((B,), torch.int64), item_len=e((B,), torch.int64),
                plan=e((runtime.JOIN_PLAN_BYTES // 8,), torch.int64))


def join(audio: Tensor, audio_len: Tensor, doc: Tensor, pos: Tensor, pause: Optional[Tensor] = None, *, num_docs: int,
         out_samples: int, bounds: Optional[Tensor] = None, gain: Optional[Tensor] = None, fade: int = 0,
         out: Optional[dict] = None) -> dict:
    """Two launches (ispk_join_plan, ispk_join_f32), no ATen compute op, no host read.  On the device: audio fp32 [B, S] (unit
    stride on S, any row stride), int64 [B] audio_len, doc (document of each item; outside [0, num_docs) drops the item), pos
    (reading position inside the document) and pause (samples behind the item, negative: overlap with the next one; None: 0);
    optional bounds int64 [B, 2] and gain fp32 [B] (an AudioConditioner's).  1 <= B, num_docs <= 1024, 0 <= fade < 2^23.
    -> dict(audio fp32 [num_docs, out_samples], audio_len, wanted_len int64 [num_docs], item_offset (-1: dropped), item_len
    int64 [B]); `out` (join_outputs) supplies them.  wanted_len > out_samples says that a document was cut."""
    for t in (audio, audio_len, doc, pos, pause, bounds, gain):
        if t is not None and not t.is_cuda:
            raise runtime.IspkError("join needs GPU tensors; there is no CPU fallback")
    if audio.ndim != 2 or audio.dtype != torch.float32 or (audio.shape[1] > 1 and audio.stride(1) != 1):
        raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                         f"{tuple(audio.stride())}")
    B, S = audio.shape
    D, S_out = int(num_docs), int(out_samples)
    if not (1 <= B <= runtime.JOIN_MAX and 1 <= D <= runtime.JOIN_MAX):
        raise ValueError(f"join: 1 .. {runtime.JOIN_MAX} items and documents per call, got B={B}, num_docs={D}")
    if not (0 <= S < 2 ** 31 and 0 <= S_out < 2 ** 31):
        raise ValueError(f"join: S={S}, out_samples={S_out}: both below 2^31")
    if int(fade) != fade or not 0 <= fade < runtime.JOIN_MAX_FADE:
        raise ValueError(f"fade is an integer in [0, 2^23), got {fade!r}")
    if B > 1 and audio.stride(0) < S:
        raise ValueError(f"audio: rows overlap (row stride {audio.stride(0)} < {S})")
    if out is None:
        out = join_outputs(D, S_out, B, audio.device)
    if out["audio"].ndim != 2:
        raise ValueError(f"out['audio']: fp32 [{D}, {S_out}], got {tuple(out['audio'].shape)}")
    runtime._out_like("out['audio']", out["audio"], torch.float32, (D, S_out))
    if D > 1 and out["audio"].stride(0) < S_out:
        raise ValueError(f"out['audio']: rows overlap (row stride {out['audio'].stride(0)} < {S_out})")
    runtime.join_plan(audio_len, doc, pos, pause, bounds, out["plan"], out["item_offset"], out["item_len"], out["audio_len"],
                      out["wanted_len"], S, S_out, int(fade))
    runtime.join_audio(audio, gain, out["plan"], out["audio_len"], out["audio"])
    return out


def marks_outputs(B: int, L: int, words: int, device) -> dict:
    """The tensors `speech_marks` fills, for a caller that keeps them (a graph capture)."""
    e = lambda shape: torch.empty(shape, dtype=torch.int64, device=device)      # noqa: E731
    return dict(token_marks=e((B, L, 2)), word_marks=e((B, int(words), 2)))


def speech_marks(duration: Tensor, text_len: Optional[Tensor], audio_len: Tensor, *, samples_per_frame: int, hard: bool = False,
                 bounds: Optional[Tensor] = None, joined: Optional[dict] = None, doc: Optional[Tensor] = None,
                 doc_bounds: Optional[Tensor] = None, word_id: Optional[Tensor] = None, words: int = 0,
                 out: Optional[dict] = None) -> dict:
    """Speech marks ("timepoints"): where every token and word lies, in samples.  One launch (ispk_speech_marks), no ATen
    compute op, no host read, integers that a numpy restatement of include/ispk.h's arithmetic reproduces exactly.  On the device:

      duration   fp32 [B, L] (unit stride on L, any row stride): what the regulator consumed - `ao.duration` of `model.infer`,
                 or the aligner's `attn_hard_duration` of a teacher-forced forward as fp32 with hard=True (forced alignment)
      text_len   int64 [B] valid tokens (None: L each);  audio_len  int64 [B] samples of the items BEFORE any trimming
      samples_per_frame   the vocoder's hop;  hard: the durations are repeats, (d + 0.5) truncated (the hard regulator's), not
                 fractional frames (the soft regulator's running fp32 sum)
      bounds     int64 [B, 2], an item conditioner's: the marks move with the trim and stay inside what is kept
      joined     the dict `join` returned (its item_offset and audio_len are used) with `doc` int64 [B], the argument `join`
                 got: the marks are then samples of the joined document; every mark of a dropped item is -1
      doc_bounds int64 [D, 2], a document conditioner's bounds on the joined documents (only with `joined`)
      word_id    int64 [B, L]: the word of each token, 0 <= id < words <= 1024; other ids (punctuation, padding) belong to no word

    -> dict(token_marks int64 [B, L, 2], word_marks int64 [B, words, 2]): (start, end) sample ranges, end exclusive; (-1, -1) for
    a token at or past text_len and for a word without a token.  Tokens of one item tile its audio.  Under a crossfade an item
    begins before its predecessor ends, so the last marks of one item and the first of the next overlap there - both are
    heard.  `out` (marks_outputs) supplies the tensors."""
    if duration.ndim != 2 or duration.dtype != torch.float32 or (duration.shape[1] > 1 and duration.stride(1) != 1):
        raise ValueError(f"duration: fp32 [B, L] with unit stride on L, got {duration.dtype} {tuple(duration.shape)} strides "
                         f"{tuple(duration.stride())}")
    B, L = duration.shape
    W, hop = int(words), int(samples_per_frame)
    if not (B <= 65535 and L <= runtime.MARKS_MAX_TOKENS and 0 <= W <= runtime.MARKS_MAX_WORDS):
        raise ValueError(f"speech_marks: B={B} (<= 65535), L={L} (<= {runtime.MARKS_MAX_TOKENS}), words={W} (<= {runtime.MARKS_MAX_WORDS})")
    if hop != samples_per_frame or not 1 <= hop <= 2 ** 20:
        raise ValueError(f"samples_per_frame is an integer in [1, 2^20], got {samples_per_frame!r}")
    if (joined is None) != (doc is None):
        raise ValueError("speech_marks: `joined` (what join returned) and `doc` (what join was given) go together")
    if doc_bounds is not None and joined is None:
        raise ValueError("speech_marks: doc_bounds only together with `joined` and `doc`")
    if word_id is not None and W == 0:
        raise ValueError("speech_marks: word_id needs words >= 1")
    for t in (duration, text_len, audio_len, bounds, doc, doc_bounds, word_id, *((joined or {}).get(k) for k in ("item_offset", "audio_len"))):
        if t is not None and not t.is_cuda:
            raise runtime.IspkError("speech_marks needs GPU tensors; there is no CPU fallback")
    if out is None:
        out = marks_outputs(B, L, W, duration.device)
    S = 2 ** 31 - 1          # the lengths are the vocoder's: nothing to hold them to but the ABI's range
    item_offset = doc_len = None
    if joined is not None:
        item_offset, doc_len = joined["item_offset"], joined["audio_len"]
        if not 1 <= doc_len.shape[0] <= runtime.JOIN_MAX:
            raise ValueError(f"speech_marks: 1 .. {runtime.JOIN_MAX} documents, got {doc_len.shape[0]}")
    runtime.speech_marks(duration, text_len, audio_len, out["token_marks"], out["word_marks"] if W else None, hop, S, bool(hard),
                         bounds, item_offset, doc, doc_len, doc_bounds, word_id)
    return out


def gain_envelope(audio: Tensor, audio_len: Tensor, token_marks: Tensor, token_gain: Tensor, *, ramp: int = 128,
                  out: Optional[Tensor] = None) -> Tensor:
    """The volume part of word-level prosody: out[b] = audio[b] * e, e the linear gain token_gain[b, l] over token l's samples
    with linear ramps of at most `ramp` samples (and at most half a token) on each side of a boundary between two tokens.  One
    launch (ispk_gain_envelope_f32; include/ispk.h has the arithmetic), no ATen compute op, no host read.  On the device:
    audio fp32 [B, S] (unit stride on S, any row stride), audio_len int64 [B], token_marks int64 [B, L, 2] in ITEM coordinates
    (`speech_marks` without bounds and without `joined`), token_gain fp32 [B, L] (`prosody_spans` builds it).  Samples at and
    past audio_len are 0 in the result.  `out` fp32 [B, S] may be `audio` itself (in place); None allocates."""
    for t in (audio, audio_len, token_marks, token_gain, out):
        if t is not None and not t.is_cuda:
            raise runtime.IspkError("gain_envelope needs GPU tensors; there is no CPU fallback")
    if audio.ndim != 2 or audio.dtype != torch.float32:
        raise ValueError(f"audio: fp32 [B, S], got {audio.dtype} {tuple(audio.shape)}")
    if out is None:
        out = torch.empty(tuple(audio.shape), dtype=torch.float32, device=audio.device)
    return runtime.gain_envelope(audio, audio_len, token_marks, token_gain, ramp, out)


PROSODY_KEYS = CONTROL_NAMES + ("gain_db",)


def prosody_spans(B: int, L: int, spans: Sequence[dict], *, base: Optional[Tensor] = None, word_id: Optional[Tensor] = None,
                  pitch_std: float = 1.0, device=None):
    """Host helper: per-token controls and gains from SSML-like spans -> (controls fp32 [B, L, 5] for `infer(controls=)`,
    gain fp32 [B, L] linear, for `gain_envelope` / `Synthesizer(prosody=True)`).

    Every row of item b starts as `base[b]` (a `make_controls` result; None: neutral) and every gain at 0 dB.  A span is a
    dict with `item=b`, then either `tokens=(first, stop)` or `words=(first, stop)` (half-open; `words` selects the tokens whose
    `word_id[b, l]` lies in the range and needs `word_id` int64 [B, L]), and any of duration_factor, pitch_factor, pitch_delta,
    energy_factor, energy_delta, gain_db.  Spans apply in order, in float64: factors multiply, deltas add (pitch_delta divided
    by `pitch_std`, as `make_controls(pitch_std=)` does), decibels add; the cast to fp32 - and gain = 10^(dB / 20) - comes last."""
    B, L = int(B), int(L)
    if base is None:
        rows = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0], dtype=torch.float64).repeat(B, 1)
    else:
        if not isinstance(base, Tensor) or tuple(base.shape) != (B, 5):
            raise ValueError(f"base: a make_controls result [{B}, 5], got {tuple(getattr(base, 'shape', ()))}")
        rows = base.detach().cpu().to(torch.float64)
    c = rows[:, None, :].repeat(1, L, 1)
    db = torch.zeros((B, L), dtype=torch.float64)
    wid = None
    if word_id is not None:
        wid = word_id.detach().cpu()
        if tuple(wid.shape) != (B, L):
            raise ValueError(f"word_id: [{B}, {L}], got {tuple(wid.shape)}")
    for n, span in enumerate(spans):
        unknown = [k for k in span if k not in PROSODY_KEYS + ("item", "tokens", "words")]
        if unknown:
            raise ValueError(f"span {n}: unknown key {unknown[0]!r} (item, tokens | words, {', '.join(PROSODY_KEYS)})")
        if "item" not in span:
            raise ValueError(f"span {n}: `item` is missing")
        b = span["item"]
        if int(b) != b or not 0 <= b < B:
            raise ValueError(f"span {n}: item {b!r} outside the batch of {B}")
        if ("tokens" in span) == ("words" in span):
            raise ValueError(f"span {n}: exactly one of `tokens` and `words`")
        key = "tokens" if "tokens" in span else "words"
        first, stop = span[key]
        if int(first) != first or int(stop) != stop or not 0 <= first <= stop:
            raise ValueError(f"span {n}: {key} range {span[key]!r} is not 0 <= first <= stop")
        if key == "tokens":
            if stop > L:
                raise ValueError(f"span {n}: tokens range {span[key]!r} outside the {L} tokens")
            sel = torch.zeros(L, dtype=torch.bool)
            sel[int(first):int(stop)] = True
        else:
            if wid is None:
                raise ValueError(f"span {n}: `words` needs word_id")
            if stop > runtime.MARKS_MAX_WORDS:
                raise ValueError(f"span {n}: words range {span[key]!r} outside the {runtime.MARKS_MAX_WORDS} words")
            sel = (wid[int(b)] >= int(first)) & (wid[int(b)] < int(stop))
        for k, v in span.items():
            if k not in PROSODY_KEYS:
                continue
            v = float(v)
            if k == "gain_db":
                db[int(b), sel] += v
                continue
            col = CONTROL_NAMES.index(k)
            if k.endswith("_factor"):
                c[int(b), sel, col] *= v
            else:
                c[int(b), sel, col] += v / float(pitch_std) if k == "pitch_delta" else v
    gain = torch.pow(torch.tensor(10.0, dtype=torch.float64), db / 20.0)
    return c.to(dtype=torch.float32, device=device), gain.to(dtype=torch.float32, device=device)


def cues(word_marks: Tensor, doc: Tensor, labels: Sequence[Sequence[str]], sample_rate: float) -> list:
    """Host helper, run after the graph: ONE device read (word_marks and doc are copied to the host here).  word_marks int64
    [B, W, 2] of `speech_marks(joined=...)`, doc int64 [B], labels[b][w] the text of word w of item b (shorter rows: the rest
    has no cue) -> [(doc, start_seconds, end_seconds, label)] sorted by (doc, start, end, item, word): document order.  Words
    without marks (-1: absent, or of a dropped item) are skipped."""
    if sample_rate <= 0:
        raise ValueError(f"sample_rate > 0, got {sample_rate!r}")
    wm, dc = word_marks.detach().cpu().tolist(), doc.detach().cpu().tolist()
    if len(labels) != len(wm) or len(dc) != len(wm):
        raise ValueError(f"cues: {len(wm)} items of marks, {len(dc)} of doc, {len(labels)} of labels")
    rows = []
    for b, (item, names) in enumerate(zip(wm, labels)):
        for w, ((start, end), name) in enumerate(zip(item, names)):
            if start >= 0:
                rows.append((dc[b], start, end, b, w, name))
    rows.sort(key=lambda r: r[:5])
    return [(d, start / sample_rate, end / sample_rate, name) for d, start, end, _, _, name in rows]


def _vtt_time(seconds: float) -> str:
    ms = int(round(seconds * 1000.0))
    return f"{ms // 3600000:02d}:{ms // 60000 % 60:02d}:{ms // 1000 % 60:02d}.{ms % 1000:03d}"


def webvtt(cues_of_one_document: Sequence[tuple]) -> str:
    """The cues of ONE document ((doc, start_seconds, end_seconds, label), as `cues` returns them) as a WebVTT file."""
    docs = {c[0] for c in cues_of_one_document}
    if len(docs) > 1:
        raise ValueError(f"webvtt: the cues of one document, got documents {sorted(docs)}")
    lines = ["WEBVTT", ""]
    for i, (_, start, end, label) in enumerate(cues_of_one_document, 1):
        text = str(label).replace("&", "&amp;").replace("<", "&lt;").replace(">", "&gt;").replace("\n", " ")
        lines += [str(i), f"{_vtt_time(start)} --> {_vtt_time(end)}", text, ""]
    return "\n".join(lines)


class SynthesisResult(dict):
    """The static outputs of a `Synthesizer` call (overwritten by the next one), and `truncated`: frames_wanted > frames, a
    device comparison made when it is read - not part of the graph."""

    def __init__(self, values: dict, frames: int):
        super().__init__(values)
        self._frames = frames

    def __getitem__(self, key):
        if key == "truncated":
            return self["frames_wanted"] > self._frames
        return super().__getitem__(key)

    @property
    def truncated(self) -> Tensor:
        return self["truncated"]


class Synthesizer:
    """Text to PCM16 documents as ONE captured HIP graph over static buffers:

        syn = Synthesizer(model, vocoder, batch=B, tokens=L, frames=M, docs=D, doc_samples=S_out, fade=64)
        r = syn(text, text_len, doc, pos, pause, controls)      # r["pcm"] int16 [D, S_out], r["audio_len"], r["truncated"], ...

    Stages: model.infer(controls=, max_dec_len=M) -> vocoder(mel, dec_lengths) -> denoiser (optional) -> the measure pass of
    `item_conditioner` (optional: its bounds and gain go straight into the join, the per-item apply pass is not run) -> join ->
    `doc_conditioner` on the joined documents (optional: document-level loudness) -> to_pcm16 -> with `marks=True` the speech
    marks (one more launch: r["token_marks"] int64 [B, L, 2] and r["word_marks"] int64 [B, words, 2], sample ranges inside the
    final documents; `word_id` int64 [B, L] of a call names each token's word, none when it is not given; the launch's other
    inputs come along as r["duration"], r["item_audio_len"], r["item_bounds"], r["joined_len"], r["doc_bounds"]).  A call copies
    With `prosody=True` (word-level prosody; `prosody_spans` builds both inputs) `controls` has one row per TOKEN - a call takes
    fp32 [B, L, 5], or [B, 5] which is copied to every token of an item - and `gain` fp32 [B, L] (None: ones) is a linear gain
    per token: behind the denoiser one `ispk_speech_marks` launch in item coordinates (r["item_token_marks"]) and one
    `gain_envelope` launch with ramps of `ramp` samples, into a buffer of its own, in front of the item conditioner.
    With `limiter=Limiter(...)` (data.condition) one ispk_limit_f32 launch on the final documents, behind `doc_conditioner` and in
    front of to_pcm16, pulls down what crossfades, gains and the document loudness pushed over the ceiling instead of leaving it
    to PCM16's clamp: r["audio"] is the limited audio, r["true_peak"] and r["reduction"] fp32 [D] say per document what came in
    and how far the gain went down; lengths and marks do not change.
    With `equalizer=Equalizer(...)` (data.equalize) one ispk_equalize_f32 call (two launches) on the item audio, behind the
    denoiser and the gain envelope and in front of `item_conditioner`'s measure pass - loudness is measured on what is heard -
    into a buffer of its own; lengths, marks and bounds do not change.  A call copies
    its arguments into the static inputs and replays; `flow_noise=None` draws new noise.  Text splitting and bucketing stay with the caller:
    one Synthesizer serves one bucket shape (B sentences of L tokens into D documents of S_out samples)."""

    def __init__(self, model, vocoder, *, batch: int, tokens: int, frames: int, docs: int, doc_samples: int, steps: int = 4,
                 denoiser=None, item_conditioner: Optional[AudioConditioner] = None,
                 doc_conditioner: Optional[AudioConditioner] = None, fade: int = 0, dither: bool = False, seed: int = 0,
                 marks: bool = False, words: int = 0, prosody: bool = False, ramp: int = 128, limiter: Optional[Limiter] = None,
                 equalizer: Optional[Equalizer] = None):
        B, L, M, D, S_out = int(batch), int(tokens), int(frames), int(docs), int(doc_samples)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise runtime.IspkError("Synthesizer needs the model on the GPU; there is no CPU fallback")
        if not (1 <= B <= runtime.JOIN_MAX and 1 <= D <= runtime.JOIN_MAX and L >= 1 and M >= 1 and 1 <= S_out < 2 ** 31):
            raise ValueError(f"Synthesizer: batch={B}, tokens={L}, frames={M}, docs={D}, doc_samples={S_out}")
        self.model, self.vocoder, self.denoiser = model, vocoder, denoiser
        self.item_conditioner, self.doc_conditioner = item_conditioner, doc_conditioner
        self.batch, self.tokens, self.frames, self.docs, self.doc_samples, self.steps = B, L, M, D, S_out, int(steps)
        self.fade, self.dither, self.seed = int(fade), bool(dither), int(seed)
        self.marks, self.words = bool(marks), int(words)
        if not 0 <= self.words <= runtime.MARKS_MAX_WORDS or (self.words and not self.marks):
            raise ValueError(f"Synthesizer: words={words} (0 .. {runtime.MARKS_MAX_WORDS}, only with marks=True)")
        if self.marks and L > runtime.MARKS_MAX_TOKENS:
            raise ValueError(f"Synthesizer: marks serve at most {runtime.MARKS_MAX_TOKENS} tokens, got {L}")
        self.prosody, self.ramp = bool(prosody), int(ramp)
        if self.prosody and L > runtime.MARKS_MAX_TOKENS:
            raise ValueError(f"Synthesizer: prosody serves at most {runtime.MARKS_MAX_TOKENS} tokens, got {L}")
        if self.prosody and (self.ramp != ramp or not 0 <= self.ramp < runtime.GAIN_MAX_RAMP):
            raise ValueError(f"Synthesizer: ramp is an integer in [0, 2^22), got {ramp!r}")
        self.multi_speaker = getattr(model, "speaker_embedding", None) is not None
        i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)      # noqa: E731
        self.static = {"text": i64(B, L), "text_len": torch.full((B,), L, dtype=torch.int64, device=dev), "doc": i64(B),
                       "pos": torch.arange(B, dtype=torch.int64, device=dev), "pause": i64(B),
                       "controls": make_controls(B, device=dev), "flow_noise": torch.randn(B, L, 3, device=dev)}
        if self.multi_speaker:
            self.static["speaker"] = i64(B)
        self._wav = vocoder.empty_outputs(B, M, dev)
        S = self._wav[0].shape[1]
        self._clean = torch.empty_like(self._wav[0]) if denoiser is not None else None
        self._item = None
        if item_conditioner is not None:
            self._item = dict(bounds=torch.empty((B, 2), dtype=torch.int64, device=dev),
                              loudness=torch.empty((B,), dtype=torch.float64, device=dev),
                              peak=torch.empty((B,), dtype=torch.float32, device=dev),
                              gain=torch.empty((B,), dtype=torch.float32, device=dev))
            item_conditioner.device_tables(dev)
        self._joined = join_outputs(D, S_out, B, dev)
        self._doc = None
        if doc_conditioner is not None:
            self._doc = doc_conditioner.empty_outputs(D, S_out, dev)
            doc_conditioner.device_tables(dev)
        if limiter is not None and not isinstance(limiter, Limiter):
            raise ValueError(f"Synthesizer: limiter is a data.Limiter or None, got {type(limiter).__name__}")
        self.limiter, self._limited = limiter, None
        if limiter is not None:      # the last fp32 stage, into a buffer of its own
            self._limited = limiter.empty_outputs(D, S_out, dev)
            limiter.device_tables(dev)
        if equalizer is not None and not isinstance(equalizer, Equalizer):
            raise ValueError(f"Synthesizer: equalizer is a data.Equalizer or None, got {type(equalizer).__name__}")
        self.equalizer, self._equalized = equalizer, None
        if equalizer is not None:    # on the item audio, into a buffer of its own
            self._equalized = equalizer.empty_outputs(B, S, dev)
            equalizer.device_tables(dev)
        self._pcm = torch.empty((D, S_out), dtype=torch.int16, device=dev)
        self._marks = None
        if self.marks or self.prosody:
            if S % M:
                raise ValueError(f"Synthesizer: marks and prosody need a vocoder with a whole hop, got {S} samples for {M} frames")
            self._hop = S // M
        self._shaped = self._item_marks = None
        if self.prosody:      # one control row and one gain per token; the envelope writes a buffer of its own
            self.static["controls"] = self.static["controls"][:, None, :].repeat(1, L, 1)
            self.static["gain"] = torch.ones((B, L), dtype=torch.float32, device=dev)
            self._item_marks = torch.empty((B, L, 2), dtype=torch.int64, device=dev)
            self._shaped = torch.empty_like(self._wav[0])
        if self.marks:
            self.static["word_id"] = torch.full((B, L), -1, dtype=torch.int64, device=dev)
            self._marks = marks_outputs(B, L, self.words, dev)
        self._graph = graph.GraphedCall(self._chain)
        self.out = self._graph.out

    def _chain(self) -> dict:
        """One eager pass over the static buffers: what the graph replays (and what a test compares a replay against)."""
        s = self.static
        with torch.no_grad():
            mel, ao = self.model.infer(s["text"], text_lengths=s["text_len"], steps=self.steps, speaker=s.get("speaker"),
                                       flow_noise=s["flow_noise"], max_dec_len=self.frames, controls=s["controls"])
            frames_wanted = self.model.temporal_adaptor.frames_wanted
            audio, audio_len = self.vocoder(mel, ao.dec_lengths, out=self._wav)
            if self.denoiser is not None:
                audio, _ = self.denoiser(audio, audio_len, out=self._clean)
            if self.prosody:
                # where every token lies in its own item (no bounds, no join), then the per-token gains over those ranges
                runtime.speech_marks(ao.duration, s["text_len"], audio_len, self._item_marks, None, self._hop, audio.shape[1],
                                     not self.model.temporal_adaptor.soft_duration)
                audio = runtime.gain_envelope(audio, audio_len, self._item_marks, s["gain"], self.ramp, self._shaped)
            if self.equalizer is not None:
                # the lengths do not change, so marks and bounds stay where they are; audio_len itself goes on
                audio = self.equalizer(audio, audio_len, out=self._equalized)["audio"]
            bounds = gain = None
            if self.item_conditioner is not None:
                c, o = self.item_conditioner, self._item
                runtime.audio_measure(audio, audio_len, c.device_tables(audio.device), c.sample_rate, c.trim_mode, c.trim_threshold,
                                      c.pad_frames, int(c.target_lufs is not None), c.target_lufs if c.target_lufs is not None else 0.0,
                                      c.peak_limit, o["bounds"], o["loudness"], o["peak"], o["gain"])
                bounds, gain = o["bounds"], o["gain"]
            j = join(audio, audio_len, s["doc"], s["pos"], s["pause"], num_docs=self.docs, out_samples=self.doc_samples,
                     bounds=bounds, gain=gain, fade=self.fade, out=self._joined)
            doc_audio, doc_len = j["audio"], j["audio_len"]
            if self.doc_conditioner is not None:
                r = self.doc_conditioner(doc_audio, doc_len, out=self._doc)
                doc_audio, doc_len = r["audio"], r["audio_len"]
            limited = None
            if self.limiter is not None:
                # the lengths do not change (no bounds here), so the marks below stay where they are
                limited = self.limiter(doc_audio, doc_len, out=self._limited)
                doc_audio = limited["audio"]
            pcm = to_pcm16(doc_audio, doc_len, dither=self.dither, seed=self.seed, out=self._pcm)
        out = dict(pcm=pcm, audio=doc_audio, audio_len=doc_len, wanted_len=j["wanted_len"], item_offset=j["item_offset"],
                   item_len=j["item_len"], frames_wanted=frames_wanted, dec_lengths=ao.dec_lengths)
        if limited is not None:
            out.update(true_peak=limited["true_peak"], reduction=limited["reduction"])
        if self.prosody:
            out["item_token_marks"] = self._item_marks
        if self.marks:
            # the last launch of the chain, fed by what the stages above consumed and wrote; its inputs are handed out too
            m, doc_bounds = self._marks, self._doc["bounds"] if self._doc is not None else None
            runtime.speech_marks(ao.duration, s["text_len"], audio_len, m["token_marks"], m["word_marks"] if self.words else None,
                                 self._hop, audio.shape[1], not self.model.temporal_adaptor.soft_duration, bounds, j["item_offset"],
                                 s["doc"], j["audio_len"], doc_bounds, s["word_id"] if self.words else None)
            out.update(token_marks=m["token_marks"], word_marks=m["word_marks"], duration=ao.duration, item_audio_len=audio_len,
                       item_bounds=bounds, joined_len=j["audio_len"], doc_bounds=doc_bounds)
        return out

    def _checked(self, name: str, t: Tensor) -> Tensor:
        want = self.static[name]
        if name == "controls" and self.prosody and isinstance(t, Tensor) and t.ndim == 2:
            want = want[:, 0]                         # [B, 5]: one row per item, copied to all of its tokens
        if not isinstance(t, Tensor):
            raise ValueError(f"{name}: a tensor {tuple(want.shape)} {want.dtype}")
        if not t.is_cuda:
            raise runtime.IspkError(f"Synthesizer needs GPU tensors ({name} is on the CPU); there is no CPU fallback")
        if tuple(t.shape) != tuple(want.shape) or t.dtype != want.dtype:
            raise ValueError(f"{name}: the captured bucket takes {want.dtype} {tuple(want.shape)}, got {t.dtype} {tuple(t.shape)}")
        return t

    def __call__(self, text: Tensor, text_len: Tensor, doc: Tensor, pos: Tensor, pause: Optional[Tensor] = None,
                 controls: Optional[Tensor] = None, speaker: Optional[Tensor] = None,
                 flow_noise: Optional[Tensor] = None, word_id: Optional[Tensor] = None,
                 gain: Optional[Tensor] = None) -> SynthesisResult:
        given = {"text": text, "text_len": text_len, "doc": doc, "pos": pos}
        if gain is not None:
            if not self.prosody:
                raise ValueError("gain: the Synthesizer was built without prosody (prosody=True)")
            given["gain"] = gain
        if word_id is not None:
            if not self.words:
                raise ValueError("word_id: the Synthesizer was built without words (marks=True, words=W)")
            given["word_id"] = word_id
        for name, t in (("pause", pause), ("controls", controls), ("flow_noise", flow_noise)):
            if t is not None:
                given[name] = t
        if speaker is not None:
            if not self.multi_speaker:
                raise ValueError("speaker: the model has no speaker table")
            given["speaker"] = speaker
        for name, t in given.items():
            self._checked(name, t)
        for name, t in given.items():
            self.static[name].copy_(t[:, None, :] if t.ndim + 1 == self.static[name].ndim else t)
        if pause is None:
            self.static["pause"].zero_()
        if controls is None:
            d = self._default_controls()
            self.static["controls"].copy_(d[:, None, :] if self.prosody else d)
        if self.prosody and gain is None:
            self.static["gain"].fill_(1.0)
        if flow_noise is None:
            self.static["flow_noise"].normal_()
        if self.marks and word_id is None:
            self.static["word_id"].fill_(-1)
        return SynthesisResult(self._graph.replay(), self.frames)

    def _default_controls(self) -> Tensor:
        d = getattr(self, "_defaults", None)
        if d is None:
            d = self._defaults = make_controls(self.batch, device=self.static["controls"].device)
        return d
