"""GPU: the noise reducer (data.NoiseReducer: csrc/noise.hip, ispk_noise_profile_f64 and ispk_noise_reduce_f32) against the
float64 restatement of tests/noise_reference.py.

Signals: tone bursts of amplitude 0.3 (three harmonics of 220 Hz) between pauses, white noise of 1e-3 everywhere, another seed
per item.

Reduce, with a given profile (the reference's for a longer signal of the same kind, so the short lengths are exercised too).
Lengths (TS = ispk_noise_tile_samples()): 0, 1, 512, 513, 514, 767, 768, 769, 1024, 1025, TS - 1, TS, TS + 1, 2 TS + 255, each
alone at the default smoothing and in three ragged batches of at most 5 at (smooth_frames, smooth_bins) = (0, 0) - the tile
alone -, (2, 2) and (1, 8) - the halo; padded row strides, NaN behind n, a sentinel behind S in `out`.  Bound (DESIGN.md 4.13,
4.21, tests/test_gpu_denoiser.py): max |out - ref64| <= 1e-4 x max |ref64| per item.  over = 1 and reduce_db = 12 put the share
of (frame, bin) cells whose raw gain sits at the floor at 0.64 .. 0.69 on these items (asserted to lie in [0.2, 0.8] for every
item of at least 3 frames, on the reference alone), so both branches of the gain are exercised, and the output differs from the
input by more than 1e-3 of the peak.
Measured on gfx950: worst max |err| / peak 2.88e-7 alone (1.40e-7 .. 2.88e-7 over the lengths) and 3.14e-7 in the batches
(2.81e-7 at (0, 0), 2.88e-7 at (2, 2), 3.14e-7 at (1, 8)); torch's own fp32 stft / istft chain around a float64 gain on the
same inputs, on the CPU: 1.78e-7 to 2.92e-7.

Profile.  Lengths TS - 1, TS, TS + 1, 2 TS + 255, 3 TS + 100 with pauses that straddle the edges of the tiles of 16 frames, an
item whose only pause is shorter than 2 guard + 1 frames (no profile) and an all-zero item (a profile of zeros).  noise_frames,
frames and flags with ==; what makes that sound is asserted first: no frame power within a relative 1e-9 of the threshold
(segmenter_reference.margin).  noise by the screen's ltas convention (tests/test_gpu_screen.py): max_k |delta| over the largest
bin, and the worst per-bin relative error, each within 8 x what torch.stft in fp32 on the CPU shows against the same float64
reference, summed over the same frames.
Measured on gfx950: max |delta| over the largest bin 1.06e-7 .. 1.50e-7 (torch 9.6e-8 .. 1.14e-7), worst per-bin relative error
2.3e-7 .. 5.3e-7 (torch 2.2e-7 .. 3.8e-7): 0.165 and 0.198 of the bounds.

Then bit identity (ragged batch = alone; padding, row stride and S; lengths out of range; repeated calls; a graph replay; the
index mapping; flagged items copied), the chain behind the Segmenter, and profile + apply as one HIP graph without ATen compute."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import noise_reference as R
from isp_tts_amd import graph, runtime
from isp_tts_amd.data import NoiseReducer, Segmenter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_REL = 1e-4
TS = runtime.NOISE_TILE_SAMPLES
LENGTHS = (0, 1, 512, 513, 514, 767, 768, 769, 1024, 1025, TS - 1, TS, TS + 1, 2 * TS + 255)
BATCHES = {"a": (0, 513, 1024, TS - 1, 769), "b": (1, 514, 1025, TS, 767), "c": (512, 768, TS + 1, 2 * TS + 255)}
assert sorted(n for b in BATCHES.values() for n in b) == sorted(LENGTHS)
SMOOTH = ((0, 0), (2, 2), (1, 8))
SENTINEL = 7.0
OVER, REDUCE_DB = 1.0, 12.0
FACTOR, GUARD, MIN_FRAMES = 1e-4, 2, 4
LONG = 6 * TS


def reducer(smooth=(2, 2), over=OVER):
    nr = NoiseReducer(R.RATE, top_db=40.0, min_noise_frames=MIN_FRAMES, over=over, reduce_db=REDUCE_DB, smooth_frames=smooth[0],
                      smooth_bins=smooth[1])
    assert nr.factor == FACTOR
    nr.guard_frames = GUARD
    return nr


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def host(t):
    return t.detach().cpu().numpy()


_CACHE = {}


def given_profile():
    """float64 [513]: the reference's profile of a longer signal."""
    if "profile" not in _CACHE:
        it = R.profile_item(R.make_signal(LONG, 1), LONG, LONG, FACTOR, "max", GUARD, MIN_FRAMES)
        assert it["flags"] == 0 and it["noise_frames"] >= 8 * MIN_FRAMES
        _CACHE["profile"] = it["noise"]
    return _CACHE["profile"]


def signal(n):
    """An item of n samples: a burst from sample 256 on and every 6,144 after it, so that the short items hold both."""
    if ("x", n) not in _CACHE:
        _CACHE[("x", n)] = R.make_signal(n, 2000 + n, bursts=[(s, s + 1536) for s in range(256, max(n, 257), 6144)])
    return _CACHE[("x", n)]


def reference(n, smooth):
    """The float64 output for signal(n) with the given profile, made once."""
    key = ("y", n, smooth)
    if key not in _CACHE:
        _CACHE[key] = R.reduce_item(signal(n), given_profile(), OVER, 10.0 ** (-REDUCE_DB / 20.0), *smooth)
    return _CACHE[key]


def run_reduce(nr, xs, lens, noise, S, index=None, flags=None, pad_in=5, pad_out=3, fill=float("nan"), use_len=None):
    """xs: the items (float64); the rest of each row is `fill`, never to be read.  noise: [P, 513], or [513] for one row per item
    (without an index item b takes row b).  -> out [B, S] on the CPU."""
    B = len(xs)
    noise = np.tile(noise, (B, 1)) if np.ndim(noise) == 1 else noise
    a = torch.full((B, S + pad_in), fill, dtype=torch.float32)
    for b, x in enumerate(xs):
        a[b, :len(x)] = torch.from_numpy(x).float()
    o = torch.full((B, S + pad_out), SENTINEL, device=DEV)
    ln = torch.tensor(lens if use_len is None else use_len, dtype=torch.int64, device=DEV)
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)      # noqa: E731
    got, n = nr.apply(a.to(DEV)[:, :S], ln, torch.from_numpy(np.atleast_2d(noise)).to(DEV), i32(index), i32(flags), out=o[:, :S])
    torch.cuda.synchronize()
    assert got.data_ptr() == o.data_ptr() and n is ln
    assert (o[:, S:] == SENTINEL).all(), "columns past S were written"
    return o[:, :S].cpu()


def check_item(got, x, want, what):
    """One item's row against float64: the bound below n, exact zeros from n on, a bit copy below 513 samples."""
    n = len(x)
    assert (got[n:] == 0).all(), f"{what}: non-zero samples at or past n"
    if n < R.MIN_SAMPLES:
        assert torch.equal(got[:n], torch.from_numpy(x).float()), f"{what}: a short item is copied bit for bit"
        return 0.0
    peak = float(np.abs(want).max())
    err = float(np.abs(got[:n].double().numpy() - want).max())
    print(f"{what}: max |err| / peak = {err / peak:.3e}")
    assert err <= FP32_REL * peak, f"{what}: max |err| {err:.3e} > 1e-4 x peak {peak:.3e}"
    return err / peak


def check_conditions(n, smooth):
    """On the reference alone: both branches of the gain are exercised and the output is not the input."""
    if n >= R.MIN_SAMPLES:                                  # (513 samples are 3 frames)
        x = signal(n)
        share = R.floor_share(x, given_profile(), OVER, 10.0 ** (-REDUCE_DB / 20.0))
        assert 0.2 <= share <= 0.8, f"n={n}: {share:.2f} of the raw gains sit at the floor"
        assert float(np.abs(reference(n, smooth) - x).max()) > 1e-3 * float(np.abs(x).max())


# ------------------------------------------------------------------------------------------------ reduce against float64
@pytest.mark.parametrize("n", LENGTHS)
def test_reduce_against_float64_alone(n):
    assert runtime.lib().ispk_noise_tile_samples() == TS and TS % 256 == 0
    x, smooth = signal(n), (2, 2)
    check_conditions(n, smooth)
    got = run_reduce(reducer(smooth), [x], [n], given_profile(), n + 37)
    rel = check_item(got[0], x, reference(n, smooth), f"alone n={n}")
    if n >= R.MIN_SAMPLES:
        want = reference(n, smooth)
        tch = float(np.abs(R.torch_reduce(x, given_profile(), OVER, 10.0 ** (-REDUCE_DB / 20.0), *smooth) - want).max() / np.abs(want).max())
        print(f"reduce alone n={n}: max|err| / peak = {rel:.2e} (torch fp32 chain on the CPU: {tch:.2e})")


@pytest.mark.parametrize("smooth", SMOOTH)
@pytest.mark.parametrize("name", list(BATCHES))
def test_reduce_against_float64_ragged(name, smooth):
    lens = BATCHES[name]
    S = max(lens) + 129
    xs = [signal(n) for n in lens]
    got = run_reduce(reducer(smooth), xs, lens, given_profile(), S)
    worst = 0.0
    for b, n in enumerate(lens):
        check_conditions(n, smooth)
        worst = max(worst, check_item(got[b], xs[b], reference(n, smooth), f"batch {name} {smooth} n={n}"))
    print(f"reduce batch {name} {lens} smoothing {smooth}: worst max|err| / peak = {worst:.2e}")


def test_over_zero_is_a_round_trip():
    lens = (513, 769, TS + 1, 100)
    xs = [signal(n) if n in LENGTHS else R.make_signal(n, n) for n in lens]
    back = run_reduce(reducer(over=0.0), xs, lens, given_profile(), TS + 200)
    for b, n in enumerate(lens):
        check_item(back[b], xs[b], xs[b], f"over 0 n={n}")


# ------------------------------------------------------------------------------------------------ profile against the reference
PROFILE_BURSTS = [(256, 1280), (5700, 6800), (9400, 10800)]
PROFILE_LENGTHS = (TS - 1, TS, TS + 1, 2 * TS + 255, 3 * TS + 100)


def profile_cases():
    """(names, audio float64 [B, S] holding fp32 values, lens, want: has a profile)."""
    if "cases" not in _CACHE:
        S = 3 * TS + 160
        names, rows, lens, want = [], [], [], []
        for n in PROFILE_LENGTHS:
            names.append(f"n{n}"), rows.append(R.make_signal(n, 3000 + n, bursts=PROFILE_BURSTS)), lens.append(n), want.append(True)
        # the only pause, samples [1500, 3100), holds three inactive frames: fewer than 2 guard + 1
        names.append("narrow"), rows.append(R.make_signal(TS, 7, bursts=[(0, 1500), (3100, TS)])), lens.append(TS), want.append(False)
        names.append("zeros"), rows.append(np.zeros(TS)), lens.append(TS), want.append(True)
        names.append("short"), rows.append(R.make_signal(512, 8, bursts=[])), lens.append(512), want.append(False)
        names.append("empty"), rows.append(np.zeros(0)), lens.append(0), want.append(False)
        audio = np.zeros((len(rows), S))
        for b, x in enumerate(rows):
            audio[b, :len(x)] = x
        items, ref = R.profile_batch(audio, lens, FACTOR, "max", GUARD, MIN_FRAMES)
        _CACHE["cases"] = dict(names=names, audio=audio, lens=np.array(lens, np.int64), want=want, items=items, ref=ref, S=S)
    return _CACHE["cases"]


def profile_error(got, ref):
    d = np.abs(got - ref)
    return float(d.max() / ref.max()), float((d / ref).max())


def run_profile(nr, audio, lens, ld_extra=4, fill=float("nan"), shift=0):
    """audio float64 [B, S] -> the profile's outputs; rows at a stride above S, `fill` behind every item and between the rows."""
    B, S = audio.shape
    LD = (S + 3) // 4 * 4 + ld_extra
    flat = torch.full((B * LD + shift,), fill, device=DEV)
    full = flat[shift:].view(B, LD)
    a = torch.from_numpy(audio).float()
    for b in range(B):
        n = int(lens[b]) if 0 <= int(lens[b]) <= S else 0
        full[b, :n] = a[b, :n].to(DEV)
    p = nr.profile(full[:, :S], torch.as_tensor(lens, dtype=torch.int64).to(DEV))
    torch.cuda.synchronize()
    return p


def test_profile_against_reference():
    c = profile_cases()
    for b, name in enumerate(c["names"]):                   # what makes == sound, and what every item is meant to be
        m, thr = R.margin(c["audio"][b], int(c["lens"][b]), FACTOR, "max")
        assert m > 1e-9, (name, m)
        it = c["items"][b]
        assert (it["flags"] == 0) == c["want"][b], (name, it["flags"], it["noise_frames"])
        if c["want"][b]:
            assert it["noise_frames"] >= MIN_FRAMES, name
    narrow = c["items"][c["names"].index("narrow")]
    p = R.frame_powers(R.hop_sums(c["audio"][c["names"].index("narrow")], TS))
    assert 0 < int((p <= narrow_threshold(p)).sum()) < 2 * GUARD + 1 and narrow["noise_frames"] == 0
    for n, edges in ((2 * TS + 255, (16,)), (3 * TS + 100, (16, 32))):     # noise frames on both sides of a tile edge (16 frames a tile)
        mask = c["items"][c["names"].index(f"n{n}")]["mask"]
        assert all(mask[e - 1] and mask[e] for e in edges), n
    got = run_profile(reducer(), c["audio"], c["lens"])
    assert set(got) == {"noise", "noise_frames", "frames", "flags"}
    assert got["noise"].dtype == torch.float64 and got["noise"].shape == (len(c["names"]), 513)
    for k in ("noise_frames", "frames", "flags"):
        assert got[k].dtype == torch.int32 and np.array_equal(host(got[k]), c["ref"][k]), (k, host(got[k]), c["ref"][k])
    noise = host(got["noise"])
    worst = [0.0, 0.0]
    for b, name in enumerate(c["names"]):
        it = c["items"][b]
        if it["flags"] or not it["noise"].any():
            assert not noise[b].any(), name
            continue
        n = it["n"]
        e_all, e_bin = profile_error(noise[b], it["noise"])
        t_all, t_bin = profile_error(R.torch_profile(c["audio"][b, :n], it["mask"]), it["noise"])
        print(f"profile {name}: {it['noise_frames']} noise frames; max |delta| over the largest bin {e_all:.3e} (torch fp32 stft {t_all:.3e}), "
              f"worst per-bin relative error {e_bin:.3e} (torch {t_bin:.3e})")
        worst = [max(worst[0], e_all / (8 * t_all)), max(worst[1], e_bin / (8 * t_bin))]
    print(f"profile: of the bounds (8 x torch's fp32 stft) at worst {worst[0]:.3f} over the largest bin, {worst[1]:.3f} per bin")
    assert max(worst) <= 1.0, worst


def narrow_threshold(p):
    return R.threshold(p, FACTOR, "max")


def test_profile_bits_and_lengths_out_of_range():
    c = profile_cases()
    nr = reducer()
    base = run_profile(nr, c["audio"], c["lens"])
    keys = ("noise", "noise_frames", "frames", "flags")
    for other in (run_profile(nr, c["audio"], c["lens"]),                                   # again
                  run_profile(nr, c["audio"], c["lens"], ld_extra=9, fill=1e30, shift=1),   # scalar loads, other padding
                  run_profile(nr, np.pad(c["audio"], ((0, 0), (0, 777))), c["lens"])):      # another S
        for k in keys:
            assert bits(other[k]) == bits(base[k]), k
    for b, name in enumerate(c["names"]):                                                   # alone, cut to its own length
        n = max(int(c["lens"][b]), 1)
        one = run_profile(nr, c["audio"][b:b + 1, :n], c["lens"][b:b + 1])
        for k in keys:
            assert bits(one[k][0]) == bits(base[k][b]), (name, k)
    S = c["S"]
    bad = run_profile(nr, c["audio"][:3], np.array([-1, S + 1, 0]))
    empty = c["names"].index("empty")
    for k in keys:
        for b in range(3):
            assert bits(bad[k][b]) == bits(base[k][empty]), k
    assert (host(bad["flags"]) == 3).all() and not host(bad["noise"]).any()


# ------------------------------------------------------------------------------------------------ bit identity of the reduce
def test_ragged_batch_equals_alone_and_ignores_padding():
    lens = (513, TS, 2 * TS + 255, 1, 1025)
    S = 2 * TS + 300
    xs = [signal(n) for n in lens]
    for smooth in ((2, 2), (1, 8)):
        nr = reducer(smooth)
        base = run_reduce(nr, xs, lens, given_profile(), S)
        for b, n in enumerate(lens):                                           # an item alone, in a shorter row
            alone = run_reduce(nr, [xs[b]], [n], given_profile(), n + 3, pad_in=2, pad_out=1)
            assert torch.equal(alone[0, :n], base[b, :n]), f"n={n}: the batch changed an item's bits"
        for fill in (0.0, 1e30):                                               # base ran with NaN past the lengths
            assert torch.equal(run_reduce(nr, xs, lens, given_profile(), S, fill=fill), base), f"fill {fill}"
        assert torch.equal(run_reduce(nr, xs, lens, given_profile(), S), base)         # a second call
        assert torch.equal(run_reduce(nr, xs, lens, given_profile(), S + 41, pad_in=8, pad_out=6)[:, :S], base)   # S and the strides
        bad = run_reduce(nr, xs, lens, given_profile(), S, use_len=(-1, TS, S + 1, 1, 1025))
        assert (bad[0] == 0).all() and (bad[2] == 0).all() and torch.equal(bad[1], base[1]) and torch.equal(bad[4], base[4])


def test_index_mapping():
    """Two rows that share a profile row get the bits of separate calls; -1 and P copy."""
    lens = (TS + 1, 1025, TS + 1, 769, 1025)
    S = TS + 64
    xs = [signal(n) for n in lens]
    other = R.profile_item(R.make_signal(LONG, 2, sigma=1.5e-3), LONG, LONG, FACTOR, "max", GUARD, MIN_FRAMES)["noise"]
    noise = np.stack([given_profile(), other])
    nr = reducer()
    mixed = run_reduce(nr, xs, lens, noise, S, index=[1, 0, 0, -1, 2])
    for b, row in ((0, 1), (1, 0), (2, 0)):
        alone = run_reduce(nr, [xs[b]], [lens[b]], noise[row], lens[b] + 5)
        assert torch.equal(mixed[b, :lens[b]], alone[0, :lens[b]]) and (mixed[b, lens[b]:] == 0).all(), b
    assert not torch.equal(mixed[0], mixed[2])                                 # the same item under two profiles
    for b in (3, 4):
        assert torch.equal(mixed[b, :lens[b]], torch.from_numpy(xs[b]).float()) and (mixed[b, lens[b]:] == 0).all(), b
    want = R.reduce_batch(np.stack([np.pad(x, (0, S - len(x))) for x in xs]), lens, noise, OVER, nr.g_min, 2, 2, index=[1, 0, 0, -1, 2])
    for b in range(3):
        check_item(mixed[b], xs[b], want[b, :lens[b]], f"index, item {b}")
    flagged = run_reduce(nr, xs, lens, noise, S, index=[1, 0, 0, 0, 0], flags=[0, 1, 2, 3, 4])
    assert torch.equal(flagged[0], mixed[0]) and not torch.equal(flagged[4, :1025], torch.from_numpy(xs[4]).float())
    for b in (1, 2, 3):
        assert torch.equal(flagged[b, :lens[b]], torch.from_numpy(xs[b]).float()) and (flagged[b, lens[b]:] == 0).all(), b


class Spy(TorchDispatchMode):
    """Records every ATen op that touches a GPU tensor, views and allocations apart."""
    HARMLESS = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.slice", "aten.select", "aten.detach", "aten.alias",
                "aten.is_", "aten.size", "aten.stride", "aten.sym_", "aten.empty_like", "aten.new_empty")

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_flatten
        out = func(*args, **(kwargs or {}))
        if not str(func).startswith(self.HARMLESS):
            if any(t.is_cuda for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)):
                self.seen.append(str(func))
        return out


def test_whole_call_flags_copy_no_aten_op_and_graph_replay():
    """nr(...) = profile + apply: the items with a profile are reduced with their own, the flagged ones ("narrow": no_profile,
    "short", "empty") come back bit for bit; one HIP graph, no ATen compute op, replays repeat the eager bits."""
    c = profile_cases()
    B, S = c["audio"].shape
    audio = torch.from_numpy(c["audio"]).float().to(DEV)
    lens = torch.from_numpy(c["lens"]).to(DEV)
    nr = reducer()
    eager = {k: v.clone() for k, v in nr(audio, lens).items()}
    torch.cuda.synchronize()
    assert set(eager) == {"audio", "audio_len", "noise", "noise_frames", "frames", "flags"}
    y, noise = eager["audio"].cpu(), host(eager["noise"])
    for b, name in enumerate(c["names"]):
        n, it = int(c["lens"][b]), c["items"][b]
        x = c["audio"][b, :n]
        if it["flags"]:
            assert torch.equal(y[b, :n], torch.from_numpy(x).float()) and (y[b, n:] == 0).all(), name
        elif name != "zeros":
            want = R.reduce_item(x, noise[b], OVER, nr.g_min, 2, 2)
            check_item(y[b], x, want, f"whole call, {name}")
            assert float(np.abs(want - x).max()) > 1e-3 * float(np.abs(x).max())
        else:
            assert not y[b].any()
    out = nr.empty_outputs(B, DEV, samples=S)
    spy = Spy()
    with spy:
        r = nr(audio, lens, out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert all(r[k] is out[k] for k in ("audio", "noise", "noise_frames", "frames", "flags"))
    for k in eager:
        assert bits(r[k]) == bits(eager[k]), k
    static = nr.empty_outputs(B, DEV, samples=S)
    g = graph.GraphedCall(lambda: nr(audio, lens, out=static))
    for _ in range(2):
        for k in ("audio", "noise", "noise_frames", "frames", "flags"):
            static[k].fill_(3)
        torch.cuda.synchronize()
        spy = Spy()
        with spy:
            r = g.replay()
        torch.cuda.synchronize()
        assert spy.seen == [], spy.seen
        for k in eager:
            assert bits(r[k]) == bits(eager[k]), k
    rows = nr.manifest(eager, c["names"])
    assert [row["flags"] for row in rows][-4:] == [("no_profile",), (), ("no_profile", "short"), ("no_profile", "short")]
    assert rows[0]["noise_frames"] == c["items"][0]["noise_frames"] and -10.0 < rows[0]["noise_db"] < -4.0 and rows[-3]["noise_db"] is None


# ------------------------------------------------------------------------------------------------ behind the segmenter
def test_segmenter_rows_reduced_with_their_recordings_profile():
    n0, n1 = 5 * TS + 300, 4 * TS
    recs = [R.make_signal(n0, 41), R.make_signal(n1, 42, sigma=1.5e-3)]
    S = n0 + 20
    rec = torch.zeros((2, S))
    for b, x in enumerate(recs):
        rec[b, :len(x)] = torch.from_numpy(x).float()
    rec, rec_len = rec.to(DEV), torch.tensor([n0, n1], dtype=torch.int64, device=DEV)
    nr = reducer()
    seg = Segmenter(R.RATE, top_db=40.0, max_segments=8, drop=())
    seg.min_silence_frames, seg.pad_frames, seg.target_samples, seg.max_samples, seg.min_samples = 6, 2, 3000, 2 * TS, 0
    p = nr.profile(rec, rec_len)
    r = seg(rec, rec_len, rows=10, samples=2 * TS)
    y, n = nr.apply(r["audio"], r["audio_len"], p["noise"], index=r["item"])
    torch.cuda.synchronize()
    assert n is r["audio_len"] and not host(p["flags"]).any()
    used, item, lens = int(r["rows"][0]), host(r["item"]), host(r["audio_len"])
    assert 4 <= used < 10 and set(item[:used]) == {0, 1} and (item[used:] == -1).all()
    rows = host(r["audio"]).astype(np.float64)
    want = R.reduce_batch(rows, lens, host(p["noise"]), OVER, nr.g_min, 2, 2, index=item)
    for row in range(10):
        check_item(y[row].cpu(), rows[row, :lens[row]], want[row, :lens[row]], f"row {row} of recording {item[row]}")
    assert not host(y[used:]).any()
