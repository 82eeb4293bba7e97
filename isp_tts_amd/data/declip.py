"""Declipper: the clipped takes that the Screen finds (flag bit 1) need not be dropped.  The samples of the runs at the rail are
restored on the GPU (csrc/declip.hip) by Janssen's AR interpolation (Janssen, Veldhuis & Vries 1986): per window an AR model of
the signal, then the unknown samples that minimise its prediction error, never inside the rail - behind the Segmenter / Screen
and in front of the AudioConditioner.  The reference has no counterpart: its corpus arrives curated.

    screen, dc = Screen(22050), Declipper()
    s = screen(audio, audio_len)
    r = dc(audio, audio_len, flags=s["flags"])                # r["audio"], r["restored"], r["dense"], r["peak"], r["flags"], ...
    dc.manifest(r, names)                                     # host rows: name, the counts, peak, flag names
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import torch
from torch import Tensor

from .. import runtime

__all__ = ["Declipper"]

KEYS = ("audio",) + tuple(name for name, _, _ in runtime.DECLIP_OUTPUTS)


class Declipper:
    """Restore the clipped samples of every item: four launches of ispk_declip_f64 with no ATen compute op, no atomics and no host
    read.  A non-finite sample is read as 0 and copied through unchanged.

    dc = Declipper(rail="max", rail_ratio=0.999, min_run=3, order=32, iterations=3)
    r = dc(audio, audio_len, flags=None, out=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride, S <= runtime.CONDITION_MAX_SAMPLES) and int64 [B] on the
                         GPU; a length n outside [0, S] counts as 0
      flags              None or the Screen's r["flags"], int32 [B]: an item without bit 1 (clipped) is copied bit for bit and gets
                         the flag 4 - Screen -> Declipper costs a copy on clean items
      r["audio"]         fp32 [B, S]: the restored samples are the float64 values rounded once; every other sample below n keeps
                         its bits; zeros from n on.  Out of place only: out["audio"] overlapping the input is a ValueError
      r["audio_len"]     int64 [B]: n
      r["thr"]           fp32 [B]: the Screen's threshold - the fp32 product peak * rail_ratio (rail="max") or fp32(rail); a sample
                         is at the rail when |x| >= thr > 0, a run is a maximal stretch of at-rail samples of one sign
      r["clip_samples"]  int64 [B]: the unknown samples, those of the runs of at least min_run (1 .. 64) samples; the Screen's
                         clip_samples for equal settings
      r["restored"]      int64 [B]: the samples replaced
      r["windows"], r["dense"]   int32 [B]: the segments of 512 samples solved, and those left as they are because their window of
                         1,024 samples holds more than runtime.DECLIP_MAX_UNKNOWNS unknown samples (or an intermediate result was
                         not finite).  A segment without unknown samples counts in neither
      r["peak"]          fp32 [B]: max |r["audio"]|, exact.  A restored peak may exceed 1: the AudioConditioner / Limiter come after
      r["flags"]         int32 [B], bits runtime.DECLIP_FLAGS: 1 restored (restored > 0), 2 dense (dense > 0), 4 skipped
    order (1 .. 32) is the AR model's, iterations (1 .. 8) the passes of model and solve over a window.  out:
    `empty_outputs(B, device, samples=S)`, allocated outside a graph capture.  An item's results depend on that item alone - not
    on B, S, the row strides or what lies behind n; repeated calls and graph replays are bit-identical."""

    def __init__(self, rail: Union[str, float] = "max", rail_ratio: float = 0.999, min_run: int = 3, order: int = 32, iterations: int = 3):
        if not (rail == "max" or (not isinstance(rail, str) and rail > 0 and math.isfinite(rail))):
            raise ValueError(f'rail is "max" or a positive finite level, got {rail!r}')
        if not 0 < rail_ratio <= 1:
            raise ValueError(f"0 < rail_ratio <= 1, got {rail_ratio!r}")
        for name, v, top in (("min_run", min_run, runtime.DECLIP_MAX_RUN), ("order", order, runtime.DECLIP_MAX_ORDER),
                             ("iterations", iterations, runtime.DECLIP_MAX_ITERATIONS)):
            if int(v) != v or not 1 <= v <= top:
                raise ValueError(f"{name} is an integer in [1, {top}], got {v!r}")
        self.rail = rail if rail == "max" else float(rail)
        self.rail_ratio, self.min_run, self.order, self.iterations = float(rail_ratio), int(min_run), int(order), int(iterations)

    def empty_outputs(self, B: int, device=None, samples: Optional[int] = None) -> dict:
        """Every tensor a call writes.  "audio" and the scratch "work" depend on S: with samples=S they are made here, else the
        first call with this dict adds them (a warm-up call in front of a graph capture does)."""
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)       # noqa: E731
        out = {name: e((B,), dt) for name, dt, _ in runtime.DECLIP_OUTPUTS}
        if samples is not None:
            out["audio"] = e((B, int(samples)), torch.float32)
            out["work"] = e((max(runtime.declip_workspace_bytes(B, int(samples)), 8),), torch.uint8)
        return out

    def _checked(self, audio: Tensor, audio_len: Tensor, flags: Optional[Tensor]) -> None:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        if audio.shape[1] > runtime.CONDITION_MAX_SAMPLES:
            raise ValueError(f"audio: at most {runtime.CONDITION_MAX_SAMPLES} samples an item, got {tuple(audio.shape)}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if flags is not None and (flags.dtype != torch.int32 or flags.shape != (audio.shape[0],)):
            raise ValueError(f"flags: int32 [{audio.shape[0]}], got {flags.dtype} {tuple(flags.shape)}")
        if not (audio.is_cuda and audio_len.is_cuda and (flags is None or flags.is_cuda)):
            raise runtime.IspkError("Declipper needs GPU tensors; there is no CPU fallback")

    def __call__(self, audio: Tensor, audio_len: Tensor, flags: Optional[Tensor] = None, out: Optional[dict] = None) -> dict:
        self._checked(audio, audio_len, flags)
        out = {} if out is None else out
        B, S = audio.shape
        if out.get("audio") is None:
            out["audio"] = torch.empty((B, S), dtype=torch.float32, device=audio.device)
        need = runtime.declip_workspace_bytes(B, S)
        w = out.get("work")
        if w is None or w.numel() < need:
            out["work"] = torch.empty((max(need, 8),), dtype=torch.uint8, device=audio.device)
        numeric = self.rail != "max"
        r = runtime.declip(audio, audio_len, flags, int(numeric), self.rail if numeric else 0.0, self.rail_ratio, self.min_run,
                           self.order, self.iterations, out)
        return {k: r[k] for k in KEYS}

    def manifest(self, r: dict, names: Sequence[str]) -> list:
        """One dict per item, in order: name, every output but the audio as a Python number and the names of its flags as a
        tuple.  Reads back once; text, no device work."""
        host = {k: r[k].detach().cpu().tolist() for k in KEYS if k != "audio"}
        if len(names) != len(host["flags"]):
            raise ValueError(f"{len(host['flags'])} items: {len(names)} names given")
        rows = []
        for b, name in enumerate(names):
            row = {"name": name}
            row.update({k: host[k][b] for k in host if k != "flags"})
            row["flags"] = tuple(n for n, bit in runtime.DECLIP_FLAGS.items() if host["flags"][b] & bit)
            rows.append(row)
        return rows
