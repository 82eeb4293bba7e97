"""CPU: the host model of the in-kernel dropout and of the GELU pair (tests/dropout_reference.py), before any kernel is compared
with it: known answers of the seed mixer, bit agreement with the two older mirrors of the hash, the edges of the threshold, the
statistics of the masks that consecutive seeds give (the promise the one-round hash was chosen on), the seed source's words,
the float64 GELU against torch's, and the tolerance floor of the fp32 approximations that the GPU tests build their bound on.

The statistical assertions are conditions on a fixed, deterministic set of masks, not measurements: on a superset of these
cases (p from 0.05 to 0.9, six bases) the worst statistic was 3.96 sigma."""
import itertools

import numpy as np
import pytest
import torch

import conditioning_reference as cr
import dropout_reference as dr
import griffinlim_reference as gr

N_STAT = 1 << 20
BASES = (0, 1234, 2 ** 63 + 12345)
PS = (0.1, 0.3, 0.5)
LAGS = (1, 2, 3, 4, 64, 100, 256, 1536)
WORDS = (0, 1, 2, -1, 2 ** 62)


def test_known_answers_and_the_three_mirrors_agree():
    assert dr.mix_seed(0) == 0xE220A8397B1DCDAF and dr.mix_seed(1) == 0x910A2DEC89025CC1
    idx = np.arange(100_000, dtype=np.uint32)
    far = idx + np.uint32(0xFFFF0000)                       # wraps: the element index enters modulo 2^32
    for seed in (0, 1, 1234, 2 ** 63 + 12345, 2 ** 64 - 1):
        word = dr.mix_seed(seed)
        assert word == gr.mix_seed(seed) == cr._splitmix64(seed)
        assert dr.run_seed(word, 5) == dr.mix_seed(word ^ 5)
        assert dr.unmix_seed(word) == seed and dr.mix_seed(dr.unmix_seed(seed)) == seed
        lo, hi = np.uint32(word & dr.M32), np.uint32(word >> 32)
        with np.errstate(over="ignore"):
            for i in (idx, far):
                h = dr.drop_hash(word, i)
                assert h.dtype == np.uint32
                assert np.array_equal(h, gr.drop_hash(word, i)) and np.array_equal(h, cr._mix32(i ^ lo) ^ hi)
                assert np.array_equal(dr.mix32(i), gr.mix32(i))


def test_keep_mask_indexing():
    """`first` shifts the index window, modulo 2^32; the boundary seeds put the requested hash on the requested element."""
    full = dr.keep_mask(77, 1000, 0.3)
    assert np.array_equal(dr.keep_mask(77, 400, 0.3, first=600), full[600:])
    wrap = dr.keep_mask(77, 1000, 0.3, first=2 ** 32 - 500)
    assert np.array_equal(wrap[500:], full[:500])
    assert dr.keep_mask(5, 1000, 0.0).all()
    for idx, value in ((0, 0), (200, 429496736), (65538, 2 ** 32 - 1)):
        seed = dr.seed_for_hash(idx, value)
        assert int(dr.drop_hash(dr.mix_seed(seed), np.uint32(idx))) == value


def test_drop_thresh_edges():
    assert dr.drop_thresh(0.0) == 0 and dr.drop_thresh(-0.0) == 0
    assert dr.drop_thresh(1e-12) == 1                       # on, though p 2^32 < 1: 0 would mean "off"
    assert dr.drop_thresh(0.5) == 2 ** 31
    assert dr.drop_thresh(float(np.nextafter(np.float32(1), np.float32(0)))) == 4294967040
    assert dr.drop_thresh(0.1) == int(float(np.float32(0.1)) * 2 ** 32) == 429496736
    assert dr.drop_thresh(0.1) != int(0.1 * 2 ** 32)        # the ABI's float, not Python's double
    assert dr.drop_thresh(0.3) == int(float(np.float32(0.3)) * 2 ** 32) != int(0.3 * 2 ** 32)
    assert dr.inv_keep(0.0) == 1.0 and dr.inv_keep(0.5) == 2.0
    assert dr.inv_keep(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1))) != 1.0 / 0.9


def _rate_ok(mask: np.ndarray, p: float) -> float:
    n = mask.size
    return abs(float(mask.mean()) - (1.0 - p)) / (p * (1.0 - p) / n) ** 0.5


def _ncov(a: np.ndarray, b: np.ndarray) -> float:
    """Normalised covariance of two 0/1 sequences times sqrt(n): ~ N(0, 1) for independent ones."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    a, b = a - a.mean(), b - b.mean()
    return abs(float((a * b).mean()) / (a.std() * b.std())) * a.size ** 0.5


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("p", PS)
def test_masks_of_consecutive_seeds_are_unrelated(p, base):
    """The stack hands layer li the seeds base + 2 li and base + 2 li + 1: 12 consecutive seeds, every mask at its rate, no
    pair correlated, and no mask correlated with itself at the lags of adjacent elements, a head's row and the FFN widths."""
    masks = [dr.keep_mask((base + k) & dr.M64, N_STAT, p) for k in range(12)]
    for k, m in enumerate(masks):
        assert _rate_ok(m, p) < 5.0, (p, base, k, _rate_ok(m, p))
    worst = max(_ncov(masks[i], masks[j]) for i, j in itertools.combinations(range(12), 2))
    assert worst < 5.0, (p, base, worst)
    for lag in LAGS:
        c = _ncov(masks[0][:-lag], masks[0][lag:])
        assert c < 5.0, (p, base, lag, c)


def test_seed_source_words():
    seed, p = 1234, 0.3
    plain = dr.keep_mask(seed, N_STAT, p)
    masks = [dr.keep_mask(seed, N_STAT, p, word=w) for w in WORDS]
    assert not np.array_equal(masks[0], plain)              # a source holding 0 is not "no source"
    assert np.array_equal(dr.keep_mask(seed, 4096, p, word=-1), dr.keep_mask(seed, 4096, p, word=2 ** 64 - 1))
    for a, b in itertools.combinations(masks + [plain], 2):
        assert _ncov(a, b) < 5.0 and not np.array_equal(a, b)
    for m in masks:
        assert _rate_ok(m, p) < 5.0


def test_float64_gelu_references_equal_torch():
    u = dr.finite_bf16_grid().double().requires_grad_()
    a = torch.nn.functional.gelu(u)
    a.backward(torch.ones_like(a))
    un = u.detach().numpy()
    assert np.abs(dr.gelu(un) - a.detach().numpy()).max() <= 1e-14
    assert np.abs(dr.gelu_grad(un) - u.grad.numpy()).max() <= 1e-14


def test_grid_covers_what_it_promises():
    g = dr.finite_bf16_grid()
    assert g.dtype == torch.bfloat16 and g.numel() % 4 == 0 and g.numel() % 1024 != 0 and (g.numel() // 4) % 256 != 0
    bits = g.view(torch.int16).numpy().view(np.uint16)
    assert len(set(bits.tolist())) == 2 * ((191 << 7) + 1)   # every pattern of |u| <= 2^64, once or (the padding) twice
    f = g.float()
    assert bool(torch.isfinite(f).all()) and float(f.abs().max()) == 2.0 ** 64
    assert 0x0000 in bits and 0x8000 in bits and 0x0001 in bits and 0x8001 in bits and 0x007F in bits   # zeros, denormals
    assert bool(((f.abs() > 25) & (f.abs() < 40)).any())


def test_tolerance_floor():
    """What the A&S 7.1.28 forms cost against the true functions when every operation is rounded to fp32 (no FMA): the
    floor under EPS_FAST.  Measured: 3.3e-7 max(|u|, 1) for gelu_as28 (half of erf's error per unit of |u|), 8.3e-7 for
    gelu_grad_fast (all of it)."""
    u = dr.finite_bf16_grid().float().numpy()
    u64 = u.astype(np.float64)
    fwd = float((np.abs(dr.as28_fp32(u).astype(np.float64) - dr.gelu(u64)) / np.maximum(np.abs(u64), 1.0)).max())
    bwd = float(np.abs(dr.grad_fast_fp32(u).astype(np.float64) - dr.gelu_grad(u64)).max())
    print(f"as28_fp32: max |err| / max(|u|, 1) = {fwd:.3e}; grad_fast_fp32: max |err| = {bwd:.3e}")
    assert dr.EPS_FAST == 2e-6
    assert fwd < dr.EPS_FAST / 2 and bwd < dr.EPS_FAST / 2
    assert fwd > 1.5e-7          # (common.h once claimed 1.5e-7 |x| for gelu_as28: the fp32 squarings cost several times that)
