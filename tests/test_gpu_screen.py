"""The screen on the GPU (ispk_screen_f64, data.Screen) against its numpy restatement (tests/screen_reference.py) on the items of
tests/screen_cases.py.

Integers, peak and flags with ==.  tests/test_screen_host.py asserts what makes that sound: no bin of a reference spectrum within
0.1 dB of its band threshold, |dc| at least 1e-6 from max_dc, peak away from min_peak.

Sums.  power: relative bound (n + 2) 2^-53 - the squares of fp32 values are exact in float64, so only the n - 1 additions (of
non-negative terms, in any order) and the division round.  dc: absolute bound (n + 2) 2^-53 mean|x|, the same count on terms of
either sign.

ltas against float64, two measures: max_k |delta| relative to the item's largest bin, and the worst per-bin relative error over
the bins within band_db of the peak over bins 2 .. 512.  The bound for each is 8 x what torch.stft in fp32 on the CPU shows against
the same float64 reference on the same item (the kernel's radix-4 Stockham passes and its W_2048-derived twiddles round differently
from pocketfft, and the items are a sample; the denoiser measured 0.97 x torch's chain).  test_against_reference prints the worst
ratio of each; DESIGN.md 4.31 records them."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import screen_cases as C
import screen_reference as R
from isp_tts_amd import graph, runtime
from isp_tts_amd.data import Screen, Segmenter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = tuple(R.DTYPES)
EXACT = R.INT_KEYS + ("peak",)
U = 2.0 ** -53


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def host(t):
    return t.detach().cpu().numpy()


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


def screen(config="max3"):
    rail, min_run = C.CONFIGS[config]
    s = Screen(C.RATE, rail=rail, min_run=min_run, band_db=C.BAND_DB, min_bandwidth_hz=C.MIN_BANDWIDTH_HZ, max_dc=C.MAX_DC,
               min_peak=C.MIN_PEAK)
    assert s.band_factor == C.BAND_FACTOR and s.min_band_bin == C.MIN_BAND_BIN
    s.min_dropout_samples = min_run
    return s


_DEVICE = {}


def on_device():
    """The batch on the GPU, made once: rows at a stride above S (a multiple of four floats, the base 16-byte aligned), NaN behind
    every item and between the rows."""
    if not _DEVICE:
        c = C.batch()
        B, S = c["audio"].shape
        LD = (S + 3) // 4 * 4 + 4
        full = torch.full((B, LD), float("nan"), device=DEV)
        full[:, :S] = torch.from_numpy(c["audio"]).to(DEV)
        lens = torch.from_numpy(c["lens"]).to(DEV)
        torch.cuda.synchronize()
        assert full.data_ptr() % 16 == 0 and full[:, :S].stride(0) == LD > S
        _DEVICE.update(full=full, audio=full[:, :S], lens=lens, B=B, S=S, LD=LD)
    return _DEVICE


_TORCH = {}


def torch_error(b, which="batch"):
    """(max |delta| over the largest bin, worst relative error over the bins within band_db) of torch's fp32 stft on item b against
    the float64 reference; made once per item."""
    if (which, b) not in _TORCH:
        c = C.long() if which == "long" else C.batch()
        it = C.reference("max3", which)[0][b]
        x = np.where(np.isfinite(c["clean"][b][:it["n"]]), c["clean"][b][:it["n"]], np.float32(0.0))
        _TORCH[(which, b)] = ltas_error(C.torch_ltas(x), it)
    return _TORCH[(which, b)]


def ltas_error(got, it):
    ref = it["ltas"]
    d = np.abs(got - ref)
    inside = ref >= it["level"]
    return float(d.max() / ref.max()), float((d[inside] / ref[inside]).max())


def check(got, config, rows=None, what="", which="batch"):
    """Everything against the reference of `config` (for the batch's rows `rows`); returns the worst ratios to the bounds of
    (power, dc, ltas overall, ltas in band)."""
    items, ref = C.reference(config, which)
    rows = range(len(items)) if rows is None else rows
    for k in EXACT:
        assert np.array_equal(host(got[k]), ref[k][list(rows)]), (what, config, k, host(got[k]), ref[k][list(rows)])
    worst = [0.0, 0.0, 0.0, 0.0]
    power, dc, ltas = host(got["power"]), host(got["dc"]), host(got["ltas"])
    for i, b in enumerate(rows):
        it = items[b]
        n = it["n"]
        if n == 0 or it["power"] == 0.0:
            assert power[i] == 0.0 and dc[i] == 0.0, (what, b)
        else:
            worst[0] = max(worst[0], abs(power[i] - it["power"]) / it["power"] / ((n + 2) * U))
            worst[1] = max(worst[1], abs(dc[i] - it["dc"]) / ((n + 2) * U * it["mean_abs"]))
        if it["F"] == 0 or it["top"] == 0.0:
            assert not ltas[i].any(), (what, b)
            continue
        e_all, e_band = ltas_error(ltas[i], it)
        t_all, t_band = torch_error(b, which)
        worst[2] = max(worst[2], e_all / (8 * t_all))
        worst[3] = max(worst[3], e_band / (8 * t_band))
    return worst


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_against_reference(config):
    d = on_device()
    got = screen(config)(d["audio"], d["lens"])
    torch.cuda.synchronize()
    assert set(got) == set(KEYS)
    for k, dt in R.DTYPES.items():
        assert host(got[k]).dtype == dt and got[k].shape == ((d["B"], R.BINS) if k == "ltas" else (d["B"],)), k
    worst = check(got, config)
    print(f"{config}: of the bounds at worst - power {worst[0]:.3g}, dc {worst[1]:.3g}, ltas over the largest bin {worst[2]:.3f} "
          f"(8 x torch's fp32 stft), ltas per bin within {C.BAND_DB:g} dB {worst[3]:.3f}")
    assert max(worst) <= 1.0, worst


def test_long_item():
    """513 tiles: the per-item kernels' staging of 256 tile summaries and their stride of 512 tiles go round more than once, with a
    rail run across the first staging edge and a zero run across the second."""
    c = C.long()
    it = C.reference("max3", "long")[0][0]
    T = C.T
    assert [r[:2] for r in it["rail_runs"]] == [(256 * T - 3, 7), (300 * T + 9, 4)] and it["clip_runs"] == 2
    assert it["dropout_runs"] == 1 and it["dropout_samples"] == 6 and it["F"] > 512 * 16
    audio, lens = torch.from_numpy(c["audio"]).to(DEV), torch.from_numpy(c["lens"]).to(DEV)
    got = screen("max3")(audio, lens)
    torch.cuda.synchronize()
    worst = check(got, "max3", what="long", which="long")
    print(f"long: of the bounds at worst - power {worst[0]:.3g}, dc {worst[1]:.3g}, ltas over the largest bin {worst[2]:.3f}, ltas per "
          f"bin within {C.BAND_DB:g} dB {worst[3]:.3f}")
    assert max(worst) <= 1.0, worst


def test_lengths_outside_the_row_count_as_zero():
    d = on_device()
    b = C.batch()["names"].index("edges")
    audio = d["audio"][b:b + 1].expand(3, -1).contiguous()
    lens = torch.tensor([-1, d["S"] + 1, 0], dtype=torch.int64, device=DEV)
    got = screen()(audio, lens)
    empty = C.batch()["names"].index("len0")
    check(got, "max3", rows=[empty] * 3, what="outside")


def test_parts():
    """parts = 1 leaves the spectrum out (ltas zeros, band_bin -1), parts = 2 the runs; what is measured has the whole screen's bits."""
    d = on_device()
    s = screen()
    whole = s(d["audio"], d["lens"])
    levels, spectrum = s(d["audio"], d["lens"], parts=1), s(d["audio"], d["lens"], parts=2)
    torch.cuda.synchronize()
    runs = ("clip_runs", "clip_samples", "clip_longest", "dropout_runs", "dropout_samples", "dropout_longest")
    for k in KEYS:
        if k not in ("ltas", "band_bin", "flags"):
            assert bits(levels[k]) == bits(whole[k]), k
        if k not in runs + ("clip_first", "flags"):
            assert bits(spectrum[k]) == bits(whole[k]), k
    assert not host(levels["ltas"]).any() and (host(levels["band_bin"]) == -1).all()
    assert not any(host(spectrum[k]).any() for k in runs) and (host(spectrum["clip_first"]) == -1).all()
    assert np.array_equal(host(levels["flags"]), host(whole["flags"]) & ~R.FLAGS["narrow"])
    assert np.array_equal(host(spectrum["flags"]), host(whole["flags"]) & ~(R.FLAGS["clipped"] | R.FLAGS["dropout"]))


# ------------------------------------------------------------------------------------------------ bit for bit
def test_alone_permuted_strided_repeated():
    d = on_device()
    B, S, LD = d["B"], d["S"], d["LD"]
    s = screen()
    base = {k: v.clone() for k, v in s(d["audio"], d["lens"]).items()}
    again = s(d["audio"], d["lens"])
    for k in KEYS:
        assert bits(again[k]) == bits(base[k]), k
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).to(DEV)
    moved = s(d["audio"][perm].contiguous(), d["lens"][perm].contiguous())
    for k in KEYS:
        assert bits(moved[k]) == bits(base[k][perm]), k
    for b in range(B):                                                          # every item alone, cut to its own length
        n = max(int(C.batch()["lens"][b]), 1)
        one = s(d["audio"][b:b + 1, :n], d["lens"][b:b + 1])
        for k in KEYS:
            assert bits(one[k][0]) == bits(base[k][b]), (C.batch()["names"][b], k)
    # a stride that is no multiple of four floats from a base 4 bytes off a 16-byte boundary: the scalar loads
    shifted = torch.full((B * (LD + 1) + 1,), float("nan"), device=DEV)
    view = shifted[1:].view(B, LD + 1)[:, :S]
    view.copy_(d["audio"])
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 1
    other = s(view, d["lens"])
    torch.cuda.synchronize()
    for k in KEYS:
        assert bits(other[k]) == bits(base[k]), k


def test_no_aten_op_and_graph_replay():
    d = on_device()
    s = screen()
    eager = {k: v.clone() for k, v in s(d["audio"], d["lens"]).items()}
    out = s.empty_outputs(d["B"], DEV, samples=d["S"])
    spy = Spy()
    with spy:
        r = s(d["audio"], d["lens"], out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert set(r) == set(KEYS) and all(r[k] is out[k] for k in r)
    for k in r:
        assert bits(r[k]) == bits(eager[k]), k
    static = s.empty_outputs(d["B"], DEV)                                       # (the warm-up calls add "work")
    g = graph.GraphedCall(lambda: s(d["audio"], d["lens"], out=static))
    for _ in range(2):
        for k in KEYS:
            static[k].fill_(3)
        torch.cuda.synchronize()
        spy = Spy()
        with spy:
            r = g.replay()
        torch.cuda.synchronize()
        assert spy.seen == [], spy.seen
        for k in r:
            assert bits(r[k]) == bits(eager[k]), k


# ------------------------------------------------------------------------------------------------ behind the segmenter
def test_segmenter_rows_go_straight_in():
    import segmenter_cases as SC
    c = SC.small()
    audio = torch.from_numpy(np.nan_to_num(c["audio"], nan=0.0)).to(DEV)
    lens = torch.from_numpy(c["lens"]).to(DEV)
    seg = Segmenter(SC.RATE, top_db=SC.TOP_DB, max_segments=SC.K_SMALL, drop=())
    seg.pad_frames = 1
    for k, v in SC.BUDGET.items():
        setattr(seg, k, v)
    r = seg(audio, lens, rows=24, samples=40 * SC.H)
    s = Screen(SC.RATE)
    s.min_dropout_samples = 64
    got = s(r["audio"], r["audio_len"])
    torch.cuda.synchronize()
    rows, n = host(r["audio"]), host(r["audio_len"])
    assert int(r["rows"][0]) >= 16
    for row in range(24):
        it = R.screen_item(rows[row], n[row], rows.shape[1], min_dropout=64, band_factor=s.band_factor)
        for k in EXACT:
            if k != "band_bin":                                                 # (these pieces were not made to keep clear of the band threshold)
                assert host(got[k])[row] == it[k], (row, k)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    lib = runtime.lib()
    B, S = 2, 8192
    audio = torch.zeros((B, S), device=DEV)
    lens = torch.full((B,), S, dtype=torch.int64, device=DEV)
    s = Screen(C.RATE)
    tables = s.device_tables(DEV)
    out = s.empty_outputs(B, DEV, samples=S)
    for t in out.values():
        t.fill_(5)
    torch.cuda.synchronize()
    before = {k: bits(v) for k, v in out.items()}
    p = lambda k: ctypes.c_void_p(out[k].data_ptr())                            # noqa: E731
    args = dict(audio=ctypes.c_void_p(audio.data_ptr()), ld_audio=S, audio_len=ctypes.c_void_p(lens.data_ptr()),
                tables=ctypes.c_void_p(tables.data_ptr()), parts=3, rail_mode=0, rail=0.0, rail_ratio=0.999, min_run=3, min_dropout=110,
                band_factor=1e-6, min_band_bin=-1, max_dc=0.01, min_peak=0.0, **{k: p(k) for k in KEYS}, workspace=p("work"),
                workspace_bytes=out["work"].numel(), B=B, S=S, stream=None)
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    refused = [(dict(B=65536), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(S=(1 << 24) + 1), E_SHAPE), (dict(parts=0), E_SHAPE),
               (dict(parts=4), E_SHAPE), (dict(rail_mode=2), E_SHAPE), (dict(rail_ratio=0.0), E_SHAPE), (dict(rail_ratio=1.5), E_SHAPE),
               (dict(rail_mode=1, rail=0.0), E_SHAPE), (dict(rail_mode=1, rail=float("inf")), E_SHAPE), (dict(min_run=0), E_SHAPE),
               (dict(min_dropout=0), E_SHAPE), (dict(band_factor=0.0), E_SHAPE), (dict(band_factor=1.0), E_SHAPE),
               (dict(min_band_bin=-2), E_SHAPE), (dict(min_band_bin=514), E_SHAPE), (dict(max_dc=-1.0), E_SHAPE),
               (dict(min_peak=float("nan")), E_SHAPE), (dict(ld_audio=S - 1), E_SHAPE),
               (dict(workspace_bytes=runtime.screen_workspace_bytes(B, S) - 1), E_ALIGN),
               (dict(workspace=ctypes.c_void_p(out["work"].data_ptr() + 4)), E_ALIGN)]
    refused += [({k: None}, E_NULL) for k in ("audio", "audio_len", "tables", "workspace") + KEYS]
    for kw, code in refused:
        assert lib.ispk_screen_f64(*{**args, **kw}.values()) == code, kw
    assert lib.ispk_screen_f64(*{**args, "B": 0}.values()) == 0                 # a no-op
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bits(v) == before[k], k
    # and the same arguments, accepted: silence is quiet and nothing else
    assert lib.ispk_screen_f64(*args.values()) == 0
    torch.cuda.synchronize()
    assert (host(out["flags"]) == R.FLAGS["quiet"]).all() and not host(out["ltas"]).any() and (host(out["clip_first"]) == -1).all()
