"""Host model of csrc/dropout.h and of the GELU pair, written from the definitions in integer and float64 arithmetic: numpy only
(torch appears solely as the container of the bf16 grid), no GPU, no import from the package.

The dropout mask is never stored: every training kernel recomputes keep = drop_hash(word, element index) >= drop_thresh(p) with
word = mix_seed(caller's seed), or run_seed(that, the seed source's device word) while a source is set.  `keep_mask` is that
function on the host; the GPU tests take every mask from here, never from a kernel.

`as28_fp32` / `grad_fast_fp32` emulate common.h's gelu_as28 / gelu_grad_fast in numpy float32 WITHOUT fused multiply-adds.  They
are no reference for any kernel: tests/test_dropout_host.py measures them against the float64 functions to derive EPS_FAST, the
approximation's share of the GPU tests' per-element bound."""
import math

import numpy as np
import torch

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
GOLDEN = 0x9E3779B97F4A7C15
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

# |gelu_as28(u) - gelu(u)| <= EPS_FAST max(|u|, 1) and |gelu_grad_fast(u) - gelu'(u)| <= EPS_FAST.  The fp32 emulations below
# measure 3.3e-7 for the first and 8.3e-7 for the second (test_dropout_host.py::test_tolerance_floor prints the figures and
# asserts them below EPS_FAST / 2): the A&S 7.1.28 polynomial's 3e-7 on erf, amplified to 8e-7 by the fp32 rounding of q through
# four squarings; gelu carries half of erf's error per unit of |u|, the derivative all of it.  The rest of the margin is for
# the device's v_rcp_f32 and v_exp_f32 at 1 ulp each, and for its FMA contraction.
EPS_FAST = 2e-6


# ------------------------------------------------------------------------------------------------ seeds and the hash
def mix_seed(z: int) -> int:
    """splitmix64's finaliser of (z + golden ratio): the launchers' 64-bit word from the caller's seed."""
    z = (int(z) + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * C1) & M64
    z = ((z ^ (z >> 27)) * C2) & M64
    return z ^ (z >> 31)


def unmix_seed(w: int) -> int:
    """The inverse of mix_seed (every step of it is a bijection of 64-bit words): the caller's seed whose launch word is `w`.
    The boundary tests use it to put a chosen hash value on a chosen element."""
    w = int(w) & M64
    w ^= (w >> 31) ^ (w >> 62)
    w = (w * pow(C2, -1, 1 << 64)) & M64
    w ^= (w >> 27) ^ (w >> 54)
    w = (w * pow(C1, -1, 1 << 64)) & M64
    w ^= (w >> 30) ^ (w >> 60)
    return (w - GOLDEN) & M64


def run_seed(mixed: int, word: int) -> int:
    """The word a kernel uses while a seed source is set: `mixed` is the launch argument (mix_seed of the caller's seed), `word`
    the 64 bits at the source's device address when the kernel runs."""
    return mix_seed((int(mixed) ^ int(word)) & M64)


def mix32(x) -> np.ndarray:
    """"lowbias32": two multiply-xorshift rounds modulo 2^32 (computed in uint64 and reduced, so nothing wraps silently)."""
    x = np.asarray(x).astype(np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def drop_hash(word: int, idx) -> np.ndarray:
    """One round over (index ^ low seed word), the high word folded in after it.  `word`: the 64-bit launch word; idx: uint32."""
    idx = np.asarray(idx).astype(np.uint64) & np.uint64(M32)
    return mix32(idx ^ np.uint64(int(word) & M32)) ^ np.uint32((int(word) >> 32) & M32)


def drop_thresh(p: float) -> int:
    """An element is kept when its hash is >= this; 0 switches dropout off.  p is rounded to float32 first: the C ABI passes a
    `float`, and float32(0.1) 2^32 is not 0.1 2^32."""
    p32 = np.float32(p)
    if not p32 > 0:
        return 0
    t = float(p32) * 4294967296.0          # exact in float64: a 24-bit significand times a power of two
    return 4294967295 if t >= 4294967295.0 else (1 if t < 1.0 else int(t))


def inv_keep(p: float) -> float:
    """1 / (1 - p) as the launchers compute it, in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def launch_word(seed: int, word=None) -> int:
    mixed = mix_seed(int(seed) & M64)
    return mixed if word is None else run_seed(mixed, int(word) & M64)


def keep_mask(seed: int, n: int, p: float, word=None, first: int = 0) -> np.ndarray:
    """bool [n]: the keep decisions for element indices first .. first + n - 1, taken modulo 2^32.  `word`: the seed source's
    value (any Python int, taken modulo 2^64; None = no source - which is not the same as a source holding 0)."""
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(int(first) & M32)) & np.uint64(M32)
    return drop_hash(launch_word(seed, word), idx) >= np.uint32(drop_thresh(p))


def seed_for_hash(idx: int, value: int, low: int = 0x1234ABCD) -> int:
    """A caller's seed under which element `idx` hashes to exactly `value` (no seed source): the low launch word is `low`, the
    high word whatever makes the hash come out."""
    high = int(mix32(np.uint32((int(idx) ^ low) & M32))) ^ (int(value) & M32)
    return unmix_seed((high << 32) | (low & M32))


# ------------------------------------------------------------------------------------------------ GELU in float64
_erfc = np.frompyfunc(math.erfc, 1, 1)
_SQRT1_2 = math.sqrt(0.5)


def _cdf(u: np.ndarray) -> np.ndarray:
    """Phi(u) = erfc(-u / sqrt 2) / 2: erfc keeps its relative accuracy in the lower tail, where 1 + erf cancels."""
    return 0.5 * _erfc(-np.asarray(u, dtype=np.float64) * _SQRT1_2).astype(np.float64)


def gelu(u) -> np.ndarray:
    u = np.asarray(u, dtype=np.float64)
    return u * _cdf(u)


def gelu_grad(u) -> np.ndarray:
    """d gelu / du = Phi(u) + u phi(u)."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore"):
        pdf = np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return _cdf(u) + u * pdf


# ------------------------------------------------------------------------------------------------ common.h's approximations, fp32
_A = tuple(np.float32(c) for c in (0.0000430638, 0.0002765672, 0.0001520143, 0.0092705272, 0.0422820123, 0.0705230784))


def _q16(ax: np.ndarray) -> np.ndarray:
    """(1 + a1 z + .. + a6 z^6)^16 at z = |x| / sqrt 2, every operation rounded to float32; +inf from |x| ~ 25 on."""
    z = ax * np.float32(0.70710678118654752440)
    q = z * _A[0] + _A[1]
    for a in (*_A[2:], np.float32(1.0)):
        q = q * z + a
    for _ in range(4):
        q = q * q
    return q


def as28_fp32(u) -> np.ndarray:
    """gelu_as28 in numpy float32, no FMA: 0.5 x + (0.5 |x| - 0.5 |x| / q^16)."""
    x = np.asarray(u, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        ax = np.abs(x)
        r = np.float32(1.0) / _q16(ax)
        hx = np.float32(0.5) * ax
        return np.float32(0.5) * x + (hx - hx * r)


def grad_fast_fp32(u) -> np.ndarray:
    """gelu_grad_fast in numpy float32, no FMA: cdf by the same erf, pdf = exp2(-x^2 / (2 ln 2)) / sqrt(2 pi)."""
    x = np.asarray(u, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        erf_abs = np.float32(1.0) - np.float32(1.0) / _q16(np.abs(x))
        cdf = np.float32(0.5) * (np.float32(1.0) + np.where(x < 0, -erf_abs, erf_abs))
        pdf = np.float32(0.39894228040143267794) * np.exp2(np.float32(-0.72134752044448170368) * x * x)
        return (cdf + x * pdf).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the input grid
def finite_bf16_grid(max_exp: int = 64) -> torch.Tensor:
    """Every bf16 bit pattern with |u| <= 2^max_exp as a bf16 tensor: +-0, both denormal ranges, |u| > 25 where q^16 is +inf,
    and the range where exp(-u^2 / 2) underflows.  Padded by repeating values to a length that is a multiple of 4 (the kernels'
    vector width) and no multiple of 1024, so the last 256-thread block of an element-wise launch is partly idle."""
    top = (127 + max_exp) << 7                               # the pattern of +2^max_exp
    pos = np.arange(top + 1, dtype=np.int64)
    bits = np.concatenate([pos, pos | 0x8000])
    n = -(-bits.size // 4) * 4
    if n % 1024 == 0:
        n += 4
    bits = np.concatenate([bits, bits[1000:1000 + n - bits.size]])
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)
