"""CPU: the screen's host side - the reference's own properties on random recordings, the conditions that make the GPU tests'
== comparisons sound (asserted on every item those tests use), the constructor's conversions and validation, the manifest, the
argument checks of the entry points (which run before any launch) and the Python face."""
import ctypes
import math

import numpy as np
import pytest
import torch

import screen_cases as C
import screen_reference as R
from isp_tts_amd import data, runtime
from isp_tts_amd.data import Screen

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
KEYS = tuple(R.DTYPES)


# ------------------------------------------------------------------------------------------------ the reference's properties
def _recording(g):
    """Noise with plateaus at +-peak, stretches of zeros (also in front and behind) and the odd NaN, not aligned to anything."""
    n = int(g.integers(1, 9000))
    x = (0.4 * g.standard_normal(n)).clip(-0.8, 0.8).astype(np.float32)
    for _ in range(int(g.integers(0, 8))):
        s, m = int(g.integers(0, n)), int(g.integers(1, 40))
        x[s:s + m] = g.choice([-0.8, 0.8, 0.0, 0.0])
    if g.random() < 0.5:
        x[:int(g.integers(0, 50))] = 0.0
    if g.random() < 0.5:
        x[n - int(g.integers(0, 50)):] = 0.0
    if g.random() < 0.3:
        x[g.integers(0, n, 3)] = np.nan
    return x


@pytest.mark.parametrize("seed", range(24))
def test_reference_properties(seed):
    g = np.random.default_rng([11, seed])
    x = _recording(g)
    n = len(x)
    min_run, min_dropout = int(g.integers(1, 6)), int(g.integers(1, 30))
    rail = "max" if seed % 2 else 0.75
    it = R.screen_item(x, n, n, rail=rail, min_run=min_run, min_dropout=min_dropout)
    clean = np.where(np.isfinite(x), x, 0.0).astype(np.float32)
    assert it["nonfinite"] == int((~np.isfinite(x)).sum()) and it["peak"] == np.abs(clean).max()
    # the runs are disjoint, maximal, of one class, and cover exactly the at-rail (zero) samples
    at_rail = (np.abs(clean) >= it["thr"]) if it["thr"] > 0 else np.zeros(n, bool)
    for runs, member in ((it["rail_runs"], at_rail), (it["zero_runs"], clean == 0)):
        seen = np.zeros(n, bool)
        for k, (s, m, c) in enumerate(runs):
            assert m >= 1 and not seen[s:s + m].any() and member[s:s + m].all()
            assert len(set(np.sign(clean[s:s + m]))) == 1
            seen[s:s + m] = True
            if k:
                ps, pm, pc = runs[k - 1]
                assert ps + pm < s or (ps + pm == s and pc != c)                # a gap, or another sign right behind
        assert np.array_equal(seen, member)
    # the counts add up
    counted = [(s, m) for s, m, _ in it["rail_runs"] if m >= min_run]
    assert it["clip_runs"] == len(counted) and it["clip_samples"] == sum(m for _, m in counted) <= int(at_rail.sum())
    assert it["clip_longest"] == max([m for _, m, _ in it["rail_runs"]], default=0)
    assert (it["clip_runs"] > 0) == (it["clip_longest"] >= min_run) == (it["clip_first"] >= 0)
    if counted:
        assert it["clip_first"] == counted[0][0] and it["clip_longest"] >= min_run
    nz = np.flatnonzero(clean != 0)
    inner = [(s, m) for s, m, _ in it["zero_runs"] if len(nz) and nz[0] < s and s + m - 1 < nz[-1] and m >= min_dropout]
    assert it["dropout_runs"] == len(inner) and it["dropout_samples"] == sum(m for _, m in inner)
    assert it["dropout_longest"] == max([m for _, m in inner], default=0)
    assert (it["dropout_runs"] > 0) == (it["dropout_longest"] >= min_dropout)
    # Parseval between ltas and the framed power: sum_k c_k ltas[k] / 1024 = mean_f sum_j (w_j x_j)^2, c = 1, 2, .., 2, 1
    F = it["F"]
    assert F == max(0, (n - 1024) // 256 + 1) and bool(it["flags"] & R.FLAGS["short"]) == (F == 0)
    if F:
        c = np.full(R.BINS, 2.0)
        c[0] = c[-1] = 1.0
        framed = np.mean([np.sum((clean[256 * f:256 * f + 1024].astype(np.float64) * R.WINDOW) ** 2) for f in range(F)])
        assert abs(np.dot(c, it["ltas"]) / 1024 - framed) <= 1e-12 * max(framed, 1e-300)
        assert (it["band_bin"] >= 2) == (it["top"] > 0) and (it["band_bin"] == -1) == (it["top"] == 0)
    else:
        assert not it["ltas"].any() and it["band_bin"] == -1
    assert abs(it["power"] - np.mean(clean.astype(np.float64) ** 2)) <= 1e-12 * it["power"]


def test_cases_hit_every_branch():
    """What each item of the GPU tests is there for, read off the reference."""
    c = C.batch()
    T = C.T
    assert T == 4096 and runtime.SCREEN_TILE_FRAMES * 256 == T and C.S == 3 * T + 8 and len(c["names"]) <= 24
    want = {0, 1, 2, 3, 4, 5, 1023, 1024, 1279, 1280, T - 1, T, T + 1, 2 * T, 3 * T + 5}
    assert want <= set(int(n) for n in c["lens"])
    assert all(np.isnan(c["audio"][b, n:]).all() for b, n in enumerate(c["lens"]))
    its = {cfg: dict(zip(c["names"], C.reference(cfg)[0])) for cfg in C.CONFIGS}
    m3, m5, n3 = its["max3"], its["max5"], its["num3"]
    assert [it["F"] for it in (m3["len1023"], m3["len1024"], m3["len1279_dc"], m3["len1280"])] == [0, 1, 1, 2]
    for n in (2, 3, 4, 5):                                                      # the whole item one run: counted from min_run on
        assert m3[f"len{n}"]["clip_runs"] == (n >= 3) and m5[f"len{n}"]["clip_runs"] == (n >= 5) and m3[f"len{n}"]["clip_longest"] == n
    e = m3["edges"]
    assert [(s, m) for s, m, _ in e["rail_runs"]] == [(T - 2, 5), (2 * T - 4, 4), (2 * T, 6), (3 * T - 3, 5)]
    assert [k for _, _, k in e["rail_runs"]] == [1, 1, 2, 2] and e["clip_first"] == T - 2 and m5["edges"]["clip_runs"] == 3
    assert [(s, m) for s, m, _ in m3["edges_zero"]["zero_runs"]] == [(T - 2, 5), (2 * T - 4, 10), (3 * T - 3, 5)]   # zeros have no sign
    assert m3["cover"]["clip_longest"] == 2 * T + 7 and m3["cover_zero"]["dropout_longest"] == 2 * T + 7
    assert m3["ends"]["clip_runs"] == 3 and m3["ends"]["clip_first"] == 0 and m3["ends"]["rail_runs"][-1][0] + 7 == 2 * T
    assert m3["ends_zero"]["dropout_runs"] == 1 and m3["ends_zero"]["dropout_samples"] == 9         # in front and behind: padding
    assert (m3["beside"]["clip_runs"], m5["beside"]["clip_runs"], m3["beside_zero"]["dropout_runs"], m5["beside_zero"]["dropout_runs"]) == (3, 1, 3, 1)
    assert m3["beside"]["clip_first"] == 110 and m5["beside"]["clip_first"] == 130 and m3["beside"]["rail_runs"][-1][:2] == (T - 3, 2)
    assert (m3["plateau"]["clip_runs"], m3["plateau"]["clip_longest"], n3["plateau"]["clip_runs"], n3["plateau"]["clip_samples"]) == (0, 1, 2, 12)
    z = m3["all_zero"]
    assert z["flags"] == R.FLAGS["quiet"] and z["dropout_runs"] == 0 and z["band_bin"] == -1 and z["F"] > 0
    nf = m3["nonfinite"]
    assert nf["nonfinite"] == 5 and nf["flags"] & R.FLAGS["nonfinite"] and nf["clip_longest"] == 4 and np.isfinite(nf["ltas"]).all()
    assert m3["len1279_dc"]["flags"] == R.FLAGS["dc"] and m3["len0"]["flags"] == R.FLAGS["quiet"] | R.FLAGS["short"]
    for cut in C.BAND_CUTS:
        it = m3[f"band{cut}"]
        assert cut <= it["band_bin"] <= min(cut + 6, 512) and bool(it["flags"] & R.FLAGS["narrow"]) == (cut < C.MIN_BAND_BIN)
        floor = 10 * np.log10(it["ltas"][min(cut + 40, 512)] / it["top"])
        assert cut == 512 or -95 < floor < -85                                 # the floor 90 dB down
    flags = 0
    for cfg in its.values():
        for it in cfg.values():
            flags |= it["flags"]
    assert flags == sum(R.FLAGS.values())


def test_margins():
    """The conditions under which the GPU's integers can be compared with ==.  No bin of a reference spectrum lies within 0.1 dB of
    its band threshold, at 60 dB (the tests') and at 40: torch's own fp32 stft moves the bins above -60 dB by a few 1e-5 relative
    (some 1e-4 dB; printed below) and the kernel is held to 8 x that, so 0.1 dB is asserted to be at least a hundred times what
    the kernel may move a bin, and torch's fp32 chain gives the reference's band_bin.  |dc| lies at least 1e-6 from max_dc - ten orders above the (n + 2) 2^-53 the sums can differ
    by.  The peak is exact, so it only has to differ from min_peak."""
    c, lo = C.batch(), C.long()
    items = C.reference("max3")[0] + C.reference("max3", "long")[0]
    worst_db, worst_move = np.inf, 0.0
    for name, x, it in zip(c["names"] + lo["names"], c["clean"] + lo["clean"], items):
        assert abs(abs(it["dc"]) - C.MAX_DC) >= 1e-6, name
        assert float(it["peak"]) != C.MIN_PEAK and abs(float(it["peak"]) - C.MIN_PEAK) >= 1e-6, name
        if it["F"] == 0 or it["top"] == 0.0:
            continue
        clean = np.where(np.isfinite(x[:it["n"]]), x[:it["n"]], np.float32(0.0))
        fp32 = C.torch_ltas(clean)
        for db in (60.0, 40.0):
            band, top, level = R.band_of(it["ltas"], it["F"], 10.0 ** (-db / 10.0))
            gap = np.abs(10.0 * np.log10(np.maximum(it["ltas"], 1e-300) / level)).min()
            assert gap >= 0.1, (name, db, gap)
            worst_db = min(worst_db, gap)
            assert R.band_of(fp32, it["F"], 10.0 ** (-db / 10.0))[0] == band, (name, db)
        inside = it["ltas"] >= it["level"]
        worst_move = max(worst_move, float((np.abs(fp32 - it["ltas"])[inside] / it["ltas"][inside]).max()))
    print(f"smallest distance of a bin to a band threshold {worst_db:.3f} dB; torch's fp32 stft moves a bin above -60 dB by at most "
          f"{worst_move:.2e} relative = {10 * math.log10(1 + worst_move):.1e} dB")
    assert 10 * math.log10(1 + 8 * worst_move) * 100 <= 0.1


# ------------------------------------------------------------------------------------------------ the constructor
def test_conversions():
    s = Screen(22050)
    assert (s.rail, s.rail_ratio, s.min_run, s.band_db, s.min_bandwidth_hz, s.max_dc, s.min_peak) == ("max", 0.999, 3, 60.0, None, 0.01, 0.0)
    assert s.min_dropout_samples == round(110.25) == 110 and s.min_band_bin == -1 and s.band_factor == 10.0 ** -6.0
    t = Screen(16000, rail=0.95, min_run=1, dropout_ms=0.0, band_db=40.0, min_bandwidth_hz=7000.0, max_dc=0.0, min_peak=0.1)
    assert t.rail == 0.95 and t.min_dropout_samples == 1 and t.min_band_bin == 448 and t.band_factor == 1e-4
    assert Screen(22050, min_bandwidth_hz=7000.0).min_band_bin == 326          # 325 * 22050 / 1024 = 6998.3 Hz is narrow, 326 is not
    assert s.bandwidth_hz(512) == 11025.0 and s.bandwidth_hz(256) == 5512.5
    assert s.tables.shape == (5120,) and s.tables.dtype == torch.float32
    assert torch.equal(s.tables[:4096], data.twiddles().flatten()) and torch.equal(s.tables[4096:], torch.hann_window(1024))
    e = s.empty_outputs(3, "cpu", samples=5000)
    assert set(e) == set(KEYS) | {"work"} and e["ltas"].shape == (3, 513) and e["flags"].shape == (3,)
    assert {k: str(v.dtype).split(".")[1] for k, v in e.items() if k != "work"} == {k: np.dtype(dt).name for k, dt in R.DTYPES.items()}
    assert e["work"].numel() == runtime.screen_workspace_bytes(3, 5000) == 8 * 3 * (524 * 2 + 1)
    assert "work" not in s.empty_outputs(3, "meta")


def test_validation():
    for kw, match in ((dict(sample_rate=0), "sample_rate"), (dict(sample_rate=22050.5), "sample_rate"), (dict(rail="peak"), "rail"),
                      (dict(rail=0.0), "rail"), (dict(rail=float("inf")), "rail"), (dict(rail_ratio=0.0), "rail_ratio"),
                      (dict(rail_ratio=1.01), "rail_ratio"), (dict(min_run=0), "min_run"), (dict(min_run=2.5), "min_run"),
                      (dict(dropout_ms=-1.0), "dropout_ms"), (dict(band_db=0.0), "band_db"), (dict(band_db=100.5), "band_db"),
                      (dict(band_db=float("nan")), "band_db"), (dict(min_bandwidth_hz=-1.0), "min_bandwidth_hz"),
                      (dict(min_bandwidth_hz=12000.0), "min_bandwidth_hz"), (dict(max_dc=-0.1), "max_dc"),
                      (dict(min_peak=float("nan")), "min_peak")):
        with pytest.raises(ValueError, match=match):
            Screen(**{"sample_rate": 22050, **kw})
    s = Screen(8000)
    a, n = torch.zeros((2, 64)), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        s(a, n)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.screen(a, n, s.tables, 0, 0.0, 0.999, 3, 110, 1e-6, -1, 0.01, 0.0)
    with pytest.raises(ValueError, match="audio"):
        s(a.double(), n)
    with pytest.raises(ValueError, match="audio"):
        s(a[:, ::2], n)
    with pytest.raises(ValueError, match="audio_len"):
        s(a, n.int())
    with pytest.raises(ValueError, match="audio_len"):
        s(a, n[:1])
    with pytest.raises(ValueError, match="samples an item"):
        s(torch.zeros((1, runtime.CONDITION_MAX_SAMPLES + 1), device="meta"), torch.zeros(1, dtype=torch.int64, device="meta"))
    for attr, bad, good in (("min_run", 0, 3), ("min_dropout_samples", 0, 5), ("min_band_bin", 514, -1)):
        setattr(s, attr, bad)
        with pytest.raises(ValueError, match=attr):
            s._checked(_Cuda(a), _Cuda(n))
        setattr(s, attr, good)
    s._checked(_Cuda(a), _Cuda(n))


class _Cuda:
    """A CPU tensor that says it is on the GPU: lets the attribute checks behind the device check run without one."""

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return True if name == "is_cuda" else getattr(self._t, name)


# ------------------------------------------------------------------------------------------------ the manifest
def test_manifest():
    s = Screen(22050)
    items, ref = C.reference("max3")
    names = C.batch()["names"]
    r = {k: torch.from_numpy(v) for k, v in ref.items()}
    rows = s.manifest(r, names)
    assert [row["name"] for row in rows] == names and list(rows[0]) == ["name"] + [k for k in KEYS if k not in ("ltas", "flags")] + ["bandwidth_hz", "flags"]
    row = rows[names.index("band186")]
    assert row["flags"] == ("narrow",) and row["bandwidth_hz"] == row["band_bin"] * 22050 / 1024 and row["clip_first"] == -1
    assert rows[names.index("len0")]["flags"] == ("quiet", "short") and rows[names.index("len0")]["bandwidth_hz"] is None
    assert rows[names.index("edges")]["flags"] == ("clipped",) and rows[names.index("edges")]["clip_runs"] == 4
    assert isinstance(row["peak"], float) and isinstance(row["clip_samples"], int)
    with pytest.raises(ValueError, match="names"):
        s.manifest(r, names[:-1])


# ------------------------------------------------------------------------------------------------ the C entry points
def _args(**kw):
    one = ctypes.c_void_p(1 << 20)                                              # never dereferenced: the checks come before any launch
    a = dict(audio=one, ld_audio=8192, audio_len=one, tables=one, parts=3, rail_mode=0, rail=0.0, rail_ratio=0.999, min_run=3,
             min_dropout=110, band_factor=1e-6, min_band_bin=-1, max_dc=0.01, min_peak=0.0, **{k: one for k in KEYS}, workspace=one,
             workspace_bytes=runtime.screen_workspace_bytes(2, 8192), B=2, S=8192, stream=None)
    a.update(kw)
    return list(a.values())


REFUSALS = [(dict(B=65536), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(S=(1 << 24) + 1), E_SHAPE), (dict(parts=0), E_SHAPE),
            (dict(parts=4), E_SHAPE), (dict(rail_mode=2), E_SHAPE), (dict(rail_mode=-1), E_SHAPE), (dict(rail_ratio=0.0), E_SHAPE),
            (dict(rail_ratio=1.5), E_SHAPE), (dict(rail_ratio=float("nan")), E_SHAPE), (dict(rail_mode=1, rail=0.0), E_SHAPE),
            (dict(rail_mode=1, rail=float("inf")), E_SHAPE), (dict(rail_mode=1, rail=float("nan")), E_SHAPE), (dict(min_run=0), E_SHAPE),
            (dict(min_dropout=0), E_SHAPE), (dict(band_factor=0.0), E_SHAPE), (dict(band_factor=1.0), E_SHAPE),
            (dict(band_factor=float("nan")), E_SHAPE), (dict(min_band_bin=-2), E_SHAPE), (dict(min_band_bin=514), E_SHAPE),
            (dict(max_dc=-1.0), E_SHAPE), (dict(max_dc=float("nan")), E_SHAPE), (dict(min_peak=-1.0), E_SHAPE),
            (dict(min_peak=float("nan")), E_SHAPE), (dict(ld_audio=8191), E_SHAPE),
            (dict(workspace_bytes=runtime.screen_workspace_bytes(2, 8192) - 1), E_ALIGN), (dict(workspace=ctypes.c_void_p((1 << 20) + 4)), E_ALIGN)
            ] + [({name: None}, E_NULL) for name in ("audio", "audio_len", "tables", "workspace") + KEYS]


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    I32, I64, F32, F64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
    assert runtime.SIGNATURES["ispk_screen_f64"] == [P, I64, P, P, I32, I32, F32, F32, I32, I32, F64, I32, F64, F64] + [P] * 15 + [I64, I32, I32, P]
    assert runtime.SIGNATURES["ispk_screen_workspace_bytes"] == [I32, I32, P] and runtime.SIGNATURES["ispk_screen_tile_samples"] == []
    assert lib.ispk_screen_tile_samples() == runtime.SCREEN_TILE_SAMPLES == 16 * 256
    n = ctypes.c_int64(-1)
    for B, S in ((0, 0), (1, 0), (1, 1), (2, 4096), (3, 4097), (7, 1 << 24), (65535, 441000)):
        assert lib.ispk_screen_workspace_bytes(B, S, ctypes.byref(n)) == 0 and n.value == runtime.screen_workspace_bytes(B, S), (B, S)
    assert lib.ispk_screen_workspace_bytes(65536, 8, ctypes.byref(n)) == E_SHAPE and lib.ispk_screen_workspace_bytes(1, 8, None) == E_NULL
    assert lib.ispk_screen_workspace_bytes(1, (1 << 24) + 1, ctypes.byref(n)) == E_SHAPE
    assert lib.ispk_screen_f64(*_args(B=0, audio=None, workspace=None)) == 0                 # a no-op: no pointer is looked at
    assert lib.ispk_screen_f64(*_args(B=0, min_run=0)) == E_SHAPE                            # the scalars are checked first
    for kw, code in REFUSALS:
        assert lib.ispk_screen_f64(*_args(**kw)) == code, kw
        assert b"ispk_screen_f64" in lib.ispk_last_error_string()


def test_python_face():
    from isp_tts_amd.bindings import audio
    names = {"screen", "screen_workspace_bytes", "SCREEN_TILE_SAMPLES", "SCREEN_TILE_FRAMES", "SCREEN_FLAGS", "SCREEN_OUTPUTS", "SCREEN_BINS"}
    assert names <= set(audio.__all__) and names <= set(runtime.__dict__)
    assert runtime.SCREEN_FLAGS == R.FLAGS == {"clipped": 1, "narrow": 2, "dc": 4, "dropout": 8, "nonfinite": 16, "quiet": 32, "short": 64}
    assert tuple(name for name, _, _ in runtime.SCREEN_OUTPUTS) == KEYS
    assert hasattr(data, "Screen") and runtime.ABI_VERSION == 2
    a, n = torch.zeros((2, 64)), torch.zeros(2, dtype=torch.int64)
    t = Screen(8000).tables
    with pytest.raises(ValueError, match="audio_len"):
        runtime.screen(a, n[:1], t, 0, 0.0, 0.999, 3, 110, 1e-6, -1, 0.01, 0.0)
    with pytest.raises(ValueError, match="tables"):
        runtime.screen(a, n, t[:100], 0, 0.0, 0.999, 3, 110, 1e-6, -1, 0.01, 0.0)
    with pytest.raises(ValueError, match="ltas"):
        runtime.screen(a, n, t, 0, 0.0, 0.999, 3, 110, 1e-6, -1, 0.01, 0.0, out=dict(ltas=torch.zeros((2, 512), dtype=torch.float64)))
    with pytest.raises(ValueError, match="work"):
        runtime.screen(a, n, t, 0, 0.0, 0.999, 3, 110, 1e-6, -1, 0.01, 0.0, out=dict(work=torch.zeros(8, dtype=torch.uint8)))
