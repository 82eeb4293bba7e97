"""Equalizer: a cascade of up to eight float64 biquads over a padded mono batch on the GPU (csrc/equalizer.hip), the stage of
the audio chain that changes the spectrum: pre- / de-emphasis around a vocoder trained on pre-emphasised audio, a rumble
high-pass in front of the loudness meter, shelves and presence peaks, a telephone band.  The reference has no counterpart.

    eq = Equalizer(22050, [highpass(80.0), peaking(3000.0, +3.0), highshelf(8000.0, -2.0)])
    r = eq(audio, audio_len)                                  # r["audio"] fp32 [B, S], r["audio_len"] int64 [B]
    Equalizer(22050, [deemphasis(0.97)])                      # behind a vocoder trained on y[n] = x[n] - 0.97 x[n-1]
    Equalizer(48000, sos=scipy.signal.butter(4, 300, "hp", fs=48000, output="sos"))

The band constructors return plain descriptions (`Band`); the Equalizer resolves them for its sample rate.  The second-order
designs are the RBJ Audio EQ Cookbook's, in float64, normalised by a0: with w0 = 2 pi f / fs, alpha = sin(w0) / (2 q), A =
10^(gain_db / 40).  `AudioConditioner` and `AudioFrontEnd` take no equalizer: call one in front of them.
"""
from __future__ import annotations

import math
from decimal import Decimal, localcontext
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .. import runtime

__all__ = ["Band", "Equalizer", "bandpass", "deemphasis", "design", "equalizer_table", "highpass", "highshelf", "lowpass",
           "lowshelf", "notch", "peaking", "preemphasis", "sos_response"]

BUTTERWORTH_Q = math.sqrt(0.5)


class Band(NamedTuple):
    """One section, before it meets a sample rate.  kind: one of KINDS; freq in Hz, gain_db and q as the kind uses them; coef
    the one-pole coefficient of the two emphasis filters."""
    kind: str
    freq: float = 0.0
    gain_db: float = 0.0
    q: float = BUTTERWORTH_Q
    coef: float = 0.0


KINDS = ("highpass", "lowpass", "bandpass", "notch", "peaking", "lowshelf", "highshelf", "preemphasis", "deemphasis")


def highpass(freq: float, q: float = BUTTERWORTH_Q) -> Band:
    """Second-order high-pass; |H| = q at freq, the Butterworth -3 dB at the default."""
    return Band("highpass", freq, 0.0, q)


def lowpass(freq: float, q: float = BUTTERWORTH_Q) -> Band:
    """Second-order low-pass; |H| = q at freq."""
    return Band("lowpass", freq, 0.0, q)


def bandpass(freq: float, q: float) -> Band:
    """Band-pass with 0 dB at freq and a bandwidth of freq / q."""
    return Band("bandpass", freq, 0.0, q)


def notch(freq: float, q: float) -> Band:
    """Notch: a zero on the unit circle at freq."""
    return Band("notch", freq, 0.0, q)


def peaking(freq: float, gain_db: float, q: float = 1.0) -> Band:
    """Bell of gain_db at freq, 0 dB at DC and at the Nyquist frequency."""
    return Band("peaking", freq, gain_db, q)


def lowshelf(freq: float, gain_db: float, q: float = BUTTERWORTH_Q) -> Band:
    """gain_db at DC, 0 dB at the Nyquist frequency, gain_db / 2 at freq."""
    return Band("lowshelf", freq, gain_db, q)


def highshelf(freq: float, gain_db: float, q: float = BUTTERWORTH_Q) -> Band:
    """gain_db at the Nyquist frequency, 0 dB at DC, gain_db / 2 at freq."""
    return Band("highshelf", freq, gain_db, q)


def preemphasis(coef: float = 0.97) -> Band:
    """y[n] = x[n] - coef x[n-1]: b = [1, -coef, 0], a = [1, 0, 0]."""
    return Band("preemphasis", coef=coef)


def deemphasis(coef: float = 0.97) -> Band:
    """y[n] = x[n] + coef y[n-1], the inverse of `preemphasis`: b = [1, 0, 0], a = [1, -coef, 0]."""
    return Band("deemphasis", coef=coef)


def design(band: Band, sample_rate: int) -> np.ndarray:
    """float64 [5] = (b0, b1, b2, a1, a2) with a0 = 1 of one band at `sample_rate`.  ValueError for an unknown kind, a
    non-finite value, q <= 0 or a frequency outside (0, sample_rate / 2)."""
    if not isinstance(band, Band) or band.kind not in KINDS:
        raise ValueError(f"a band is made by one of {', '.join(KINDS)}, got {band!r}")
    if not all(isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v) for v in band[1:]):
        raise ValueError(f"{band.kind}: every value is a finite number, got {band!r}")
    if band.kind == "preemphasis":
        return np.array([1.0, -float(band.coef), 0.0, 0.0, 0.0])
    if band.kind == "deemphasis":
        return np.array([1.0, 0.0, 0.0, -float(band.coef), 0.0])
    if not 0.0 < band.freq < sample_rate / 2.0:
        raise ValueError(f"{band.kind}: the frequency lies in (0, {sample_rate / 2.0}) Hz at {sample_rate} Hz, got {band.freq!r}")
    if not band.q > 0.0:
        raise ValueError(f"{band.kind}: q > 0, got {band.q!r}")
    w0 = 2.0 * math.pi * float(band.freq) / float(sample_rate)
    cs, alpha = math.cos(w0), math.sin(w0) / (2.0 * float(band.q))
    A = 10.0 ** (float(band.gain_db) / 40.0)
    a = [1.0 + alpha, -2.0 * cs, 1.0 - alpha]
    if band.kind == "lowpass":
        b = [(1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0]
    elif band.kind == "highpass":
        b = [(1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0]
    elif band.kind == "bandpass":
        b = [alpha, 0.0, -alpha]
    elif band.kind == "notch":
        b = [1.0, -2.0 * cs, 1.0]
    elif band.kind == "peaking":
        b = [1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A]
        a = [1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A]
    else:
        r = 2.0 * math.sqrt(A) * alpha
        if band.kind == "lowshelf":
            b = [A * ((A + 1.0) - (A - 1.0) * cs + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), A * ((A + 1.0) - (A - 1.0) * cs - r)]
            a = [(A + 1.0) + (A - 1.0) * cs + r, -2.0 * ((A - 1.0) + (A + 1.0) * cs), (A + 1.0) + (A - 1.0) * cs - r]
        else:
            b = [A * ((A + 1.0) + (A - 1.0) * cs + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), A * ((A + 1.0) + (A - 1.0) * cs - r)]
            a = [(A + 1.0) - (A - 1.0) * cs + r, 2.0 * ((A - 1.0) - (A + 1.0) * cs), (A + 1.0) - (A - 1.0) * cs - r]
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]])


def sos_response(sos: np.ndarray, freqs, sample_rate: float) -> np.ndarray:
    """complex128: H(e^(j w)) of the cascade sos float64 [N, 5] at the frequencies `freqs` in Hz, w = 2 pi f / sample_rate."""
    z1 = np.exp(-2j * np.pi * np.asarray(freqs, dtype=np.float64) / float(sample_rate))
    h = np.ones_like(z1)
    for b0, b1, b2, a1, a2 in np.asarray(sos, dtype=np.float64):
        h = h * (b0 + (b1 + b2 * z1) * z1) / (1.0 + (a1 + a2 * z1) * z1)
    return h


TABLE_DIGITS = 100            # decimal digits of the arithmetic behind the table


def _joint_transition(sos: np.ndarray) -> list:
    """[2 N][2 N] Decimals: one step of the cascade's update with x = 0, over (s0, s1) of section 0, then of section 1, ...:
    column i is what the update makes of the i-th unit state.  Block lower-triangular."""
    n = sos.shape[0]
    zero, one = Decimal(0), Decimal(1)
    A = [[zero] * (2 * n) for _ in range(2 * n)]
    for i in range(2 * n):
        s = [one if c == i else zero for c in range(2 * n)]
        x = zero
        for k in range(n):
            b0, b1, b2, a1, a2 = (Decimal(float(v)) for v in sos[k])
            y = b0 * x + s[2 * k]
            A[2 * k][i] = -a1 * y + (b1 * x + s[2 * k + 1])
            A[2 * k + 1][i] = -a2 * y + b2 * x
            x = y
    return A


def _squared(X: list) -> list:
    n = len(X)
    return [[sum((X[i][k] * X[k][j] for k in range(n)), Decimal(0)) for j in range(n)] for i in range(n)]


def _power_chain(A: list, first: int, count: int) -> list:
    """float64 arrays [A^(2^first), A^(2^(first + 1)), ...], `count` of them, each the power of the given matrix rounded once: the
    squarings run in 100-digit decimal arithmetic.  In float64 they do not survive a low corner: its poles lie close together
    (5 Hz at 48 kHz: 0.99954 +- 0.00046 i), the transition is nearly defective, its powers grow to 1 / (1 - |pole|) before they
    decay, and a float64 squaring chain loses nine digits (A^8192 off by 3e-7 of its entries - more than the fp32 rounding of
    the output that the kernel's error bound consists of)."""
    out = []
    for e in range(first + count):
        if e >= first:
            out.append(np.array([[float(v) for v in row] for row in A]))
        A = _squared(A)
    return out


def equalizer_table(sos: np.ndarray) -> np.ndarray:
    """float64 [40 N + 4 N^2] for ispk_equalize_f32 (include/ispk.h has the layout): the coefficients, every section's
    A_k^(32 2^j), j = 0 .. 7, with A_k = [[-a1, 1], [-a2, 0]] the transition of its two transposed-direct-form-II states, and
    the joint A^8192 - powers of the float64 coefficients as they stand, each entry rounded once."""
    sos = np.asarray(sos, dtype=np.float64)
    n = sos.shape[0]
    assert runtime.EQ_CHUNK_SAMPLES == 1 << 5 and runtime.EQ_SEGMENT_SAMPLES == 1 << 13
    head = np.zeros((n, 8))
    head[:, :5] = sos
    powers = np.zeros((n, 8, 4))
    with localcontext() as ctx:
        ctx.prec = TABLE_DIGITS
        for k in range(n):
            A = [[-Decimal(float(sos[k, 3])), Decimal(1)], [-Decimal(float(sos[k, 4])), Decimal(0)]]
            powers[k] = np.stack([P.reshape(-1) for P in _power_chain(A, 5, 8)])
        joint = _power_chain(_joint_transition(sos), 13, 1)[0]
    t = np.concatenate([head.reshape(-1), powers.reshape(-1), joint.reshape(-1)])
    assert t.shape == (runtime.EQ_TABLE_DOUBLES(n),)
    return t


class Equalizer:
    """A cascade of 1 .. 8 biquads, at most two launches of ispk_equalize_f32 (csrc/equalizer.hip) with no ATen compute op
    and no host read; float64 inside, fp32 in and out.

    eq = Equalizer(sample_rate, bands=None, sos=None)         # exactly one of the two
      bands              a list of `Band`s (highpass, lowpass, bandpass, notch, peaking, lowshelf, highshelf, preemphasis,
                         deemphasis), resolved for sample_rate, run in the order given
      sos                float64 [N, 6] in scipy's layout (b0, b1, b2, a0, a1, a2) or [N, 5] = (b0, b1, b2, a1, a2) with a0 = 1
    r = eq(audio, audio_len, out=None)
      audio, audio_len   fp32 [B, S] (unit stride on S, any row stride) and int64 [B] on the GPU; a length outside [0, S] counts as 0
      r["audio"]         fp32 [B, S]: the filtered item, every state zero at its first sample, zeros from its length on
      r["audio_len"]     int64 [B]: the lengths - the ringing past the end is cut
      out                `empty_outputs(B, S, device)`: the two and the scratch "work"; out["audio"] may be `audio` itself
    `.sos` float64 [N, 5]; `.response(freqs)` complex128 on the host.  ValueError: no or more than 8 sections, a frequency
    outside (0, sample_rate / 2), q <= 0, a non-finite value, an unstable section (not |a2| < 1 and |a1| < 1 + a2)."""

    def __init__(self, sample_rate: int, bands: Optional[Sequence[Band]] = None, sos=None):
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError(f"sample_rate is a positive integer, got {sample_rate!r}")
        self.sample_rate = int(sample_rate)
        if (bands is None) == (sos is None):
            raise ValueError("Equalizer: give exactly one of bands and sos")
        if bands is not None:
            bands = [bands] if isinstance(bands, Band) else list(bands)
            rows = np.stack([design(b, self.sample_rate) for b in bands]) if bands else np.zeros((0, 5))
        else:
            rows = np.array(sos, dtype=np.float64)
            if rows.ndim != 2 or rows.shape[1] not in (5, 6):
                raise ValueError(f"sos: float64 [N, 6] (scipy's layout) or [N, 5], got {rows.shape}")
            if not np.isfinite(rows).all():
                raise ValueError("sos: every value is finite")
            if rows.shape[1] == 6:
                if (rows[:, 3] == 0.0).any():
                    raise ValueError("sos: a0 is not zero")
                rows = np.delete(rows, 3, axis=1) / rows[:, 3:4]
        if not 1 <= rows.shape[0] <= runtime.EQ_MAX_SECTIONS:
            raise ValueError(f"Equalizer: 1 .. {runtime.EQ_MAX_SECTIONS} sections, got {rows.shape[0]}")
        if not np.isfinite(rows).all():
            raise ValueError("Equalizer: every coefficient is finite")
        for k, (_, _, _, a1, a2) in enumerate(rows):
            if not (abs(a2) < 1.0 and abs(a1) < 1.0 + a2):
                raise ValueError(f"Equalizer: section {k} is unstable (a1 = {a1!r}, a2 = {a2!r}; |a2| < 1 and |a1| < 1 + a2)")
        self.sos = np.ascontiguousarray(rows)
        self.sections = int(rows.shape[0])
        self._table: Optional[Tensor] = None
        self._on: dict = {}

    @property
    def table(self) -> Tensor:
        """float64 [EQ_TABLE_DOUBLES(sections)] on the host: what ispk_equalize_f32 reads (made on first use)."""
        if self._table is None:
            self._table = torch.from_numpy(equalizer_table(self.sos))
        return self._table

    def response(self, freqs) -> np.ndarray:
        """complex128: the cascade's frequency response at `freqs` in Hz (host)."""
        return sos_response(self.sos, freqs, self.sample_rate)

    def device_tables(self, device) -> Tensor:
        """The kernel's table (float64) on `device`, copied once per device (before, not inside, a graph capture)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.table.to(device)
        return t

    def empty_outputs(self, B: int, S: int, device) -> dict:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)      # noqa: E731
        return dict(audio=e((B, S), torch.float32), audio_len=e((B,), torch.int64),
                    work=e((max(1, runtime.equalize_workspace_doubles(B, S, self.sections)),), torch.float64))

    def __call__(self, audio: Tensor, audio_len: Tensor, out: Optional[dict] = None) -> dict:
        if audio.ndim != 2 or audio.dtype != torch.float32 or audio.stride(-1) != 1:
            raise ValueError(f"audio: fp32 [B, S] with unit stride on S, got {audio.dtype} {tuple(audio.shape)} strides "
                             f"{tuple(audio.stride())}")
        if audio_len.dtype != torch.int64 or audio_len.shape != (audio.shape[0],):
            raise ValueError(f"audio_len: int64 [{audio.shape[0]}], got {audio_len.dtype} {tuple(audio_len.shape)}")
        if not (audio.is_cuda and audio_len.is_cuda):
            raise runtime.IspkError("Equalizer needs GPU tensors; there is no CPU fallback")
        if out is None:
            out = self.empty_outputs(audio.shape[0], audio.shape[1], audio.device)
        runtime.equalize(audio, audio_len, self.device_tables(audio.device), self.sections, out["audio"], out["audio_len"],
                         out.get("work"))
        return {"audio": out["audio"], "audio_len": out["audio_len"]}
