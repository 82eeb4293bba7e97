"""The trim frames are ONE definition (csrc/chunk_grid.h: the hop sums, p_t, the threshold, the ends) under three operators.
Each has its float64 reference in its own test file; this one pins from outside that the three agree with each other, on one
small ragged batch whose lengths sit on every edge of the grid: an empty item, one sample, one sample either side of a hop
(255, 256), of a frame (1,023) and of the 8,192-sample segment (8,191, 8,192, 8,193), a second workgroup with a ragged hop
(8,192 + 257), and a length above S, which every operator reads as 0.  The batch runs once at a row stride and base that allow
float4 loads and once where they forbid them (an odd stride, the base 4 bytes off a 16-byte boundary).

  * Segmenter.plan's first start and last end are AudioConditioner's (start, end), as integer arrays, at equal top_db, ref and
    pad_frames.  Every item holds one burst, so no qualifying pause lies between its first and last active frames.
  * NoiseReducer.profile's `frames` against the conditioner's frame count.  The conditioner's trim frames are t = 0 .. T - 1,
    T = ceil(n / 256) (condition.hip); the profile counts the STFT frames f = t + 2 of a centred framing, F = 1 + floor(n / 256)
    from 513 samples on and 0 below, where it flags the item short (noise.hip).  So F = T + (1 if 256 divides n else 0) for
    n >= 513, with n as the conditioner itself reads it (its `end` with trimming off).  No item is left out: below 513 samples
    (here 0, 1, 255, 256 and the length above S) the comparison is that F is 0 and the short flag is set.
"""
import numpy as np
import pytest
import torch

from isp_tts_amd.data import AudioConditioner, NoiseReducer, Segmenter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATE, TOP_DB, PAD, HOP, SEG = 22050, 40.0, 1, 256, 8192
S = SEG + 260
LENGTHS = (0, 1, 255, 256, 1023, SEG - 1, SEG, SEG + 1, SEG + 257, S + 1)
REFS = {"max": "max", "const": 1e-2}
FLAG_SHORT = 2


def host(t):
    return t.detach().cpu().numpy()


def recordings():
    """fp32 [B, S]: noise below 1e-4 with one burst of magnitudes in [0.125, 0.25] over the middle third of the item (at least
    one sample): a frame that holds a burst sample is active under either ref, with a wide margin, and no other frame is."""
    rng = np.random.default_rng(5)
    x = np.zeros((len(LENGTHS), S), np.float32)
    for b, n in enumerate(LENGTHS):
        if n > S:
            n = S                                                               # (what lies in the row of the item that reads as empty)
        amp = np.full(n, 1e-4)
        amp[n // 3:max(2 * n // 3, n // 3 + 1)] = 0.25
        x[b, :n] = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n) * amp).astype(np.float32)
    return x


def on_device(x, layout):
    """The batch with NaN behind every item and between the rows: stride and base a multiple of 16 bytes, or neither."""
    B = x.shape[0]
    LD, shift = (S + 4, 0) if layout == "float4" else (S + 5, 1)
    flat = torch.full((B * LD + shift,), float("nan"), device=DEV)
    view = flat[shift:].view(B, LD)[:, :S]
    for b, n in enumerate(LENGTHS):
        if 0 < n <= S:
            view[b, :n] = torch.from_numpy(x[b, :n]).to(DEV)
    assert (view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0) == (layout == "float4")
    return view, torch.tensor(LENGTHS, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("ref", list(REFS))
@pytest.mark.parametrize("layout", ["float4", "scalar"])
def test_three_operators_one_definition(layout, ref):
    audio, lens = on_device(recordings(), layout)
    cond = AudioConditioner(RATE, target_lufs=None, top_db=TOP_DB, pad_frames=PAD, ref=REFS[ref])
    seg = Segmenter(RATE, top_db=TOP_DB, ref=REFS[ref], max_segments=4)
    seg.pad_frames = PAD
    nr = NoiseReducer(RATE, top_db=TOP_DB, ref=REFS[ref], min_noise_frames=1)
    assert seg.factor == nr.factor == 10.0 ** (-TOP_DB / 10.0) and cond.pad_frames == seg.pad_frames == PAD

    bounds = host(cond(audio, lens)["bounds"])
    plan = {k: host(v) for k, v in seg.plan(audio, lens).items()}
    prof = {k: host(v) for k, v in nr.profile(audio, lens).items()}
    read_len = host(AudioConditioner(RATE, target_lufs=None, top_db=None)(audio, lens)["bounds"])[:, 1]
    torch.cuda.synchronize()

    # what the batch is meant to be: every length as given, the one above S as 0; real trimming on the long items
    want_len = np.array([n if n <= S else 0 for n in LENGTHS])
    assert np.array_equal(read_len, want_len)
    for b, n in enumerate(want_len):
        start, end = bounds[b]
        assert 0 <= start <= n // 3 and min(n, 2 * n // 3) <= end <= n and (end > start) == (n > 0), (n, start, end)
        if n >= SEG - 1:
            assert start > 0 and end < n, (n, start, end)

    count = plan["count"]
    assert np.array_equal(plan["wanted"], count) and (count <= 1).all() and np.array_equal(count == 1, want_len > 0)
    ends = np.zeros_like(bounds)
    for b in range(len(LENGTHS)):
        if count[b]:
            ends[b] = plan["segments"][b, 0, 0], plan["segments"][b, count[b] - 1, 1]
    assert ends.dtype == bounds.dtype == np.int64 and np.array_equal(ends, bounds), (ends, bounds)

    T = (read_len + HOP - 1) // HOP                                             # the conditioner's frame count
    want_frames = np.where(read_len >= 513, T + (read_len % HOP == 0), 0)
    assert np.array_equal(prof["frames"], want_frames), (prof["frames"], want_frames)
    assert np.array_equal((prof["flags"] & FLAG_SHORT) != 0, read_len < 513)
