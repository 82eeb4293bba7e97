"""Segmenter: long recordings cut into utterances at their pauses, batched on the GPU (csrc/segment.hip) - the first stage of
the data side and the inverse of `longform.join`.  An audiobook chapter or a studio session is minutes to hours long; everything
behind this stage is built for utterances.  The reference has no counterpart: its recordings arrive as utterances.

    seg = Segmenter(22050)                                    # pauses of 300 ms at -40 dB, pieces of 6 .. 20 s
    r = seg(audio, audio_len, rows=256)                       # r["audio"] fp32 [256, max_samples], r["audio_len"], r["item"], ...
    cond(r["audio"], r["audio_len"])                          # straight into AudioConditioner / AcousticFeatures / AudioFrontEnd
    seg.manifest(r, names)                                    # (name, index, start_s, end_s, flags) per row, for the metadata file

The frames are exactly `AudioConditioner`'s trim frames; cuts lie inside pauses, so nothing fades.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import torch
from torch import Tensor

from .. import runtime

__all__ = ["Segmenter"]

HOP, FRAME = 256, 1024
PLAN_KEYS = ("segments", "flags", "count", "wanted", "frames", "speech_frames", "speech_power", "noise_power")
ROW_KEYS = ("audio", "audio_len", "item", "index", "bounds", "row_flags", "rows", "rows_wanted")


class Segmenter:
    """Find the pauses, choose cuts so that the pieces fit a length budget, gather the pieces into a padded batch: four launches
    (two of ispk_segment_plan, two of ispk_segment_gather_f32) with no ATen compute op, no atomics and no host read.

    seg = Segmenter(sample_rate, top_db=40.0, ref="max", min_silence_ms=300.0, pad_ms=50.0, target_s=6.0, max_s=20.0, min_s=1.0,
                    max_segments=256, drop=("over", "short"))
    r = seg(audio, audio_len, rows=R, samples=None, out=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride) and int64 [B] on the GPU; a length outside [0, S] counts as 0
      rows, samples      the gathered batch is [R, samples]; samples defaults to max_samples
      the plan, [B, K] with K = max_segments, slots at or past count zero:
      r["segments"]      int64 [B, K, 2]: (start, end) of every piece, increasing and disjoint.  Frames of 1024 samples every 256
                         are active above ref * 10^(-top_db / 10) (AudioConditioner's trim frames); a pause is a run of at least
                         min_silence_frames inactive frames between the first and last active frame; the cut lies in its middle
                         and each side keeps at most pad_frames frames of it.  One greedy pass cuts at the first pause that makes
                         a piece of target_samples or more, and at the last pause that still fitted when the next would exceed
                         max_samples (include/ispk.h has the loop).
      r["flags"]         int32 [B, K]: 1 "over" - longer than max_samples, a stretch without a usable pause; 2 "short" - shorter
                         than min_samples
      r["count"], r["wanted"]   int32 [B]: pieces stored, and pieces found (wanted > K: raise max_segments)
      r["frames"], r["speech_frames"]   int32 [B, K]: frames that start inside the piece, and the active ones among them
      r["speech_power"], r["noise_power"]   float64 [B, K]: mean frame power over the active / inactive frames, 0 where there is
                         none; their ratio is the SNR estimate that dataset curation filters on
      the gathered rows, pieces with a flag named in `drop` left out, in (item, piece) order:
      r["audio"], r["audio_len"]   fp32 [R, samples], int64 [R]: the pieces bit for bit, zeros behind them
      r["item"], r["index"]   int32 [R]: the recording and the piece's index within it; item -1 for an unused row
      r["bounds"]        int64 [R, 2]: (start, end) in the recording
      r["row_flags"]     int32 [R]: the piece's flags, | 4 "cut" when it was longer than `samples`
      r["rows"], r["rows_wanted"]   int32 [1]: rows used, and what an unbounded R would have used
    seg.plan(audio, audio_len, out=None) returns the plan alone.  out: `empty_outputs(B, rows, samples, device)`, allocated
    outside a graph capture.  A piece's bits and a recording's plan depend on that recording alone; repeated calls and graph
    replays are bit-identical.  The host conversions are plain attributes (min_silence_frames >= 4, pad_frames, target_samples,
    max_samples, min_samples): a test may set small values."""

    def __init__(self, sample_rate: int, top_db: float = 40.0, ref: Union[str, float] = "max", min_silence_ms: float = 300.0,
                 pad_ms: float = 50.0, target_s: float = 6.0, max_s: float = 20.0, min_s: float = 1.0, max_segments: int = 256,
                 drop: Sequence[str] = ("over", "short")):
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
        if not (top_db > 0 and math.isfinite(top_db)):
            raise ValueError(f"top_db > 0, got {top_db!r}")
        if not (ref == "max" or (not isinstance(ref, str) and ref > 0 and math.isfinite(ref))):
            raise ValueError(f'ref is "max" or a positive number, got {ref!r}')
        for name, v in (("min_silence_ms", min_silence_ms), ("pad_ms", pad_ms), ("target_s", target_s), ("min_s", min_s)):
            if not (v >= 0 and math.isfinite(v)):
                raise ValueError(f"{name} >= 0, got {v!r}")
        if not (max_s > 0 and math.isfinite(max_s)):
            raise ValueError(f"max_s > 0, got {max_s!r}")
        if not min_s <= target_s <= max_s:
            raise ValueError(f"min_s <= target_s <= max_s, got {min_s!r}, {target_s!r}, {max_s!r}")
        if int(max_segments) != max_segments or not 1 <= max_segments <= runtime.SEGMENT_MAX_SEGMENTS:
            raise ValueError(f"max_segments is an integer in [1, {runtime.SEGMENT_MAX_SEGMENTS}], got {max_segments!r}")
        drop = (drop,) if isinstance(drop, str) else tuple(drop)
        if any(d not in ("over", "short") for d in drop):
            raise ValueError(f'drop names flags among "over" and "short", got {drop!r}')
        self.sample_rate, self.top_db = int(sample_rate), float(top_db)
        self.ref = ref if ref == "max" else float(ref)
        self.min_silence_ms, self.pad_ms = float(min_silence_ms), float(pad_ms)
        self.target_s, self.max_s, self.min_s = float(target_s), float(max_s), float(min_s)
        self.max_segments, self.drop = int(max_segments), drop
        self.factor = 10.0 ** (-self.top_db / 10.0)
        silence = int(round(self.min_silence_ms * self.sample_rate / 1000.0))
        self.min_silence_frames = max(4, (silence - FRAME) // HOP + 1)      # frames wholly inside a pause of `silence` samples
        self.pad_frames = int(round(self.pad_ms * self.sample_rate / 1000.0 / HOP))
        self.target_samples = int(round(self.target_s * self.sample_rate))
        self.max_samples = int(round(self.max_s * self.sample_rate))
        self.min_samples = int(round(self.min_s * self.sample_rate))
        if self.pad_frames > runtime.SEGMENT_MAX_PAD:
            raise ValueError(f"pad_ms {pad_ms!r} is {self.pad_frames} frames at {self.sample_rate} Hz: at most {runtime.SEGMENT_MAX_PAD}")
        if self.max_samples < 1 or self.max_samples >= 2 ** 31:
            raise ValueError(f"max_s {max_s!r} is {self.max_samples} samples at {self.sample_rate} Hz: 1 .. 2^31 - 1")

    @property
    def drop_mask(self) -> int:
        return sum(runtime.SEGMENT_FLAGS[d] for d in set(self.drop))

    def empty_outputs(self, B: int, rows: int, samples: Optional[int] = None, device=None,
                      recording_samples: Optional[int] = None) -> dict:
        """Every tensor a call writes.  The plan's scratch "work" depends on S: with recording_samples=S it is made here, else
        the first call with this dict adds it (a warm-up call in front of a graph capture does)."""
        samples = self.max_samples if samples is None else int(samples)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)      # noqa: E731
        K = self.max_segments
        work = {} if recording_samples is None else dict(
            work=e((max(runtime.segment_workspace_bytes(B, int(recording_samples)), 8),), torch.uint8))
        return dict(work, segments=e((B, K, 2), torch.int64), flags=e((B, K), torch.int32), count=e((B,), torch.int32),
                    wanted=e((B,), torch.int32), frames=e((B, K), torch.int32), speech_frames=e((B, K), torch.int32),
                    speech_power=e((B, K), torch.float64), noise_power=e((B, K), torch.float64),
                    audio=e((rows, samples), torch.float32), audio_len=e((rows,), torch.int64), item=e((rows,), torch.int32),
                    index=e((rows,), torch.int32), bounds=e((rows, 2), torch.int64), row_flags=e((rows,), torch.int32),
                    rows=e((1,), torch.int32), rows_wanted=e((1,), torch.int32))

    def _checked(self, audio: Tensor, audio_len: Tensor) -> None:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not (audio.is_cuda and audio_len.is_cuda):
            raise runtime.IspkError("Segmenter needs GPU tensors; there is no CPU fallback")
        if int(self.min_silence_frames) != self.min_silence_frames or self.min_silence_frames < 4:
            raise ValueError(f"min_silence_frames is an integer >= 4, got {self.min_silence_frames!r}")
        if int(self.pad_frames) != self.pad_frames or not 0 <= self.pad_frames <= runtime.SEGMENT_MAX_PAD:
            raise ValueError(f"pad_frames is an integer in [0, {runtime.SEGMENT_MAX_PAD}], got {self.pad_frames!r}")
        if self.max_samples < 1 or self.target_samples < 0 or self.min_samples < 0:
            raise ValueError(f"max_samples >= 1, target_samples >= 0, min_samples >= 0, got {self.max_samples!r}, "
                             f"{self.target_samples!r}, {self.min_samples!r}")

    def _work(self, out: dict, audio: Tensor) -> dict:
        """`out` with a scratch buffer large enough for `audio` (made here when a caller's dict has none or a smaller one)."""
        need = runtime.segment_workspace_bytes(audio.shape[0], audio.shape[1])
        w = out.get("work")
        if w is None or w.numel() < need:
            out["work"] = torch.empty((max(need, 8),), dtype=torch.uint8, device=audio.device)
        return out

    def plan(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        """The plan alone (two launches): segments, flags, count, wanted, frames, speech_frames, speech_power, noise_power."""
        self._checked(audio, audio_len)
        out = self._work({} if out is None else out, audio)
        r = runtime.segment_plan(audio, audio_len, self.factor, 0 if self.ref == "max" else 1, 0.0 if self.ref == "max" else self.ref,
                                 self.pad_frames, self.min_silence_frames, self.target_samples, self.max_samples, self.min_samples,
                                 self.max_segments, out)
        return {k: r[k] for k in PLAN_KEYS}

    def __call__(self, audio: Tensor, audio_len: Tensor, rows: Optional[int] = None, samples: Optional[int] = None,
                 out: Optional[dict] = None) -> dict:
        if out is not None and "audio" in out:
            rows = out["audio"].shape[0] if rows is None else rows
            samples = out["audio"].shape[1] if samples is None else samples
        if rows is None:
            raise ValueError("Segmenter: give rows=R (the gathered batch is [R, samples]) or out=empty_outputs(...)")
        samples = self.max_samples if samples is None else samples
        if int(rows) != rows or not 0 <= rows <= runtime.SEGMENT_MAX_ROWS:
            raise ValueError(f"rows is an integer in [0, {runtime.SEGMENT_MAX_ROWS}], got {rows!r}")
        if int(samples) != samples or not 0 <= samples < 2 ** 31:
            raise ValueError(f"samples is an integer in [0, 2^31), got {samples!r}")
        out = {} if out is None else out
        r = self.plan(audio, audio_len, out)
        g = runtime.segment_gather(audio, r["segments"], r["flags"], r["count"], self.drop_mask, int(rows), int(samples), out)
        r.update({k: g[k] for k in ROW_KEYS})
        return r

    def manifest(self, r: dict, names: Sequence[str], sample_rate: Optional[int] = None) -> list:
        """[(name, index, start_s, end_s, flags)] for the used rows of a result, in row order: names[item], the piece's index in
        its recording, its start and end in seconds at `sample_rate` (default: the segmenter's) and the names of its row flags
        (a tuple among "over", "short", "cut").  Reads back once; text, no device work."""
        rate = float(self.sample_rate if sample_rate is None else sample_rate)
        if not (rate > 0 and math.isfinite(rate)):
            raise ValueError(f"sample_rate > 0, got {sample_rate!r}")
        host = {k: r[k].detach().cpu().tolist() for k in ("rows", "item", "index", "bounds", "row_flags")}
        out = []
        for row in range(min(int(host["rows"][0]), len(host["item"]))):
            b = host["item"][row]
            if not 0 <= b < len(names):
                raise ValueError(f"row {row} comes from item {b}: {len(names)} names given")
            start, end = host["bounds"][row]
            flags = tuple(n for n, bit in runtime.SEGMENT_FLAGS.items() if host["row_flags"][row] & bit)
            out.append((names[b], host["index"][row], start / rate, end / rate, flags))
        return out
